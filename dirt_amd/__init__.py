"""dirt_amd -- MI355X-native drop-in for the hot path of pmh47/dirt:
`rasterise`, `rasterise_batch`, `rasterise_deferred`, `rasterise_batch_deferred` (dirt/__init__.py:2)."""
from .rasterise_ops import rasterise, rasterise_batch, rasterise_deferred, rasterise_batch_deferred  # noqa: F401
from . import rasterise_ops  # noqa: F401
from . import matrices, lighting, projection  # noqa: F401  (dirt.matrices, dirt.lighting, dirt.projection)
from . import texture  # noqa: F401  (the texture helpers of samples/textured.py)
from . import shading  # noqa: F401  (the fused G-buffer lighting of samples/deferred.py's shader)
from . import geometry  # noqa: F401  (the fused vertex stage in front of the rasteriser: transforms and vertex normals)
from .geometry import MeshTopology, vertex_stage  # noqa: F401
from . import skinning  # noqa: F401  (fused linear-blend skinning in front of the vertex stage: a blend of bone matrices per vertex)
from .skinning import SkinWeights, skin_vertices  # noqa: F401
from . import kinematics  # noqa: F401  (fused forward kinematics in front of the skinning stage: rotations and joints -> bone transforms)
from .kinematics import Skeleton, pose_skeleton  # noqa: F401
from . import blendshapes  # noqa: F401  (fused blend shapes at the head of the chain: template and coefficients -> rest vertices and joints)
from .blendshapes import BlendShapes, blend_shapes  # noqa: F401
from .graphed import GraphedStep, backward  # noqa: F401  (a training step captured once as a HIP graph: the remedy for eager autograd's host cost)
