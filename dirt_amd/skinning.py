"""Linear-blend skinning in front of the vertex stage, fused: rest-pose vertices and bone transforms -> posed vertices.
The reference's samples move a mesh with one `model` matrix per scene (samples/deferred.py:40-41); an articulated mesh
(SMPL / MANO / FLAME bodies, hands, faces) moves every vertex with a weighted blend of bone matrices.  One HIP kernel
forward, one to four backward (dirt_skin.hip; specification in DESIGN.md §7d).

    skin = SkinWeights(bone_indices, bone_weights, num_bones)   # once per mesh: the inverted index the bone gradient walks
    skin = SkinWeights.from_dense(weights_VJ)                   # or from an SMPL-style dense [V, J] matrix
    for it in range(n):
        posed = skin_vertices(vertices, skin, bone_transforms)
        clip, world, normals = dirt_amd.vertex_stage(posed, topology, model, view_projection)

The scatter of the bone gradient (outer(v, g) added into [B, J, 4, 4]: float atomics on a few dozen addresses in a torch
composition) is a gather over the inverted index here: no atomics, and the same bits on every run.
"""
import torch

from . import _lib
from . import _stage

# Entries of a chunk of the inverted index: the bone-gradient kernel gives one workgroup of 256 lanes to every (chunk,
# scene), so a bone named by n entries is spread over ceil(n / CHUNK) workgroups: four entries per lane.  Measured (the last
# block of tools/bench_skinning.py): 256 to 4096 time alike where a step is bound by its launches, and at
# V = 75 000, B = 8, where the bone sums are the longest kernel, 1024 is the quickest (63 us against 64.5 to 68.6).  A
# SkinWeights keeps the value it was built with.
CHUNK = 1024


class SkinWeights(_stage.StageIndex):
    """The skinning weights of a mesh and the inverted index of their bone indices, built once.

    bone_indices: int32 / int64 [V, K], bone_weights: float32 [V, K], 1 <= K <= 8, on any one device; num_bones: J.
    Weights are taken as given: nothing is renormalised, a zero weight is padding, and a vertex may name one bone in two
    slots (both count).  An index outside [0, J), another shape or dtype raise ValueError (this reads one value back from
    the device; `skin_vertices` never does).
    Attributes (int32 unless noted, on the device of `bone_indices`):
        bone_indices [V, K]; bone_weights [V, K] float32;
        entries [V K]: the positions v * K + k ordered by bone, then position; offsets [J + 1]: the entries of bone j are
        entries[offsets[j]:offsets[j + 1]];
        chunk_table [chunks, 3]: (bone, begin, end) -- every bone's run of `entries` cut into pieces of `chunk` entries
        (the last of a bone shorter), none spanning two bones; chunk_offsets [J + 1]: the chunks of bone j are
        chunk_table[chunk_offsets[j]:chunk_offsets[j + 1]].  A bone no vertex names has no entries and no chunk.
    """

    def __init__(self, bone_indices, bone_weights, num_bones, chunk=None):
        K_MAX = _lib.SKIN_MAX_INFLUENCES
        if not isinstance(bone_indices, torch.Tensor) or bone_indices.dim() != 2 or not 1 <= bone_indices.shape[1] <= K_MAX:
            raise ValueError('SkinWeights expects bone_indices [V, K] with 1 <= K <= %d, got %s' % (K_MAX, tuple(getattr(bone_indices, 'shape', ())),))
        if bone_indices.dtype not in (torch.int32, torch.int64):
            raise ValueError('SkinWeights expects int32 or int64 bone_indices, got %s' % bone_indices.dtype)
        if not isinstance(bone_weights, torch.Tensor) or bone_weights.shape != bone_indices.shape:
            raise ValueError('SkinWeights expects bone_weights shaped like bone_indices %s, got %s'
                             % (tuple(bone_indices.shape), tuple(getattr(bone_weights, 'shape', ())),))
        if bone_weights.dtype != torch.float32:
            raise ValueError('SkinWeights expects float32 bone_weights, got %s' % bone_weights.dtype)
        if bone_weights.device != bone_indices.device:
            raise ValueError('SkinWeights: bone_weights is on %s, bone_indices on %s' % (bone_weights.device, bone_indices.device))
        if isinstance(num_bones, bool) or not isinstance(num_bones, int) or num_bones < 0:
            raise ValueError('SkinWeights expects num_bones >= 0, got %r' % (num_bones,))
        chunk = CHUNK if chunk is None else chunk
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError('SkinWeights expects chunk >= 1, got %r' % (chunk,))
        V, K = (int(s) for s in bone_indices.shape)
        if V > _lib.SKIN_MAX_VERTICES or num_bones > _lib.SKIN_MAX_BONES:
            raise ValueError('SkinWeights: at most %d vertices and %d bones' % (_lib.SKIN_MAX_VERTICES, _lib.SKIN_MAX_BONES))
        if V * K > _lib.SKIN_MAX_ENTRIES:   # the positions v * K + k and the chunks' (begin, end) are int32
            raise ValueError('SkinWeights: %d vertices x %d influences, at most %d entries' % (V, K, _lib.SKIN_MAX_ENTRIES))
        dev = bone_indices.device
        flat = bone_indices.reshape(-1).long()   # position v * K + k
        _stage.check_index_range(flat, num_bones, 'SkinWeights: bone_indices name bones %d..%d, outside [0, %d)')
        # a stable sort of the positions by bone keeps every bone's entries in order of position
        entries = torch.argsort(flat, stable=True).to(torch.int32)
        offsets = _stage.sort_offsets(flat, num_bones)
        per_bone = (torch.diff(offsets) + (chunk - 1)) // chunk
        bone = torch.repeat_interleave(torch.arange(num_bones, device=dev), per_bone)             # the bone of every chunk
        chunk_offsets = _stage.sort_offsets(bone, num_bones)
        begin = offsets[bone] + (torch.arange(bone.numel(), device=dev) - chunk_offsets[bone]) * chunk
        end = torch.minimum(begin + chunk, offsets[bone + 1])
        self.num_vertices, self.num_bones, self.influences, self.chunk = V, num_bones, K, chunk
        self.num_chunks = int(bone.numel())
        self.bone_indices, self.bone_weights = bone_indices.to(torch.int32).contiguous(), bone_weights.detach().contiguous()
        self.entries, self.offsets = entries.contiguous(), offsets.to(torch.int32)
        self.chunk_table = torch.stack([bone, begin, end], 1).to(torch.int32).contiguous()
        self.chunk_offsets = chunk_offsets.to(torch.int32)

    _TENSORS = ('bone_indices', 'bone_weights', 'entries', 'offsets', 'chunk_table', 'chunk_offsets')

    @classmethod
    def from_dense(cls, weights, chunk=None):
        """From an SMPL-style dense matrix, float32 [V, J]: the non-zero entries of every row in order of bone.  K is the
        largest count of non-zero entries in a row (at least 1; more than 8 raises ValueError); shorter rows are padded
        with bone 0 and weight 0."""
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.dtype != torch.float32:
            raise ValueError('SkinWeights.from_dense expects float32 weights [V, J], got %s %s'
                             % (getattr(weights, 'dtype', type(weights).__name__), tuple(getattr(weights, 'shape', ())),))
        V, J = (int(s) for s in weights.shape)
        nonzero = weights != 0
        K = max(int(nonzero.sum(1).max()) if V and J else 0, 1)
        if K > _lib.SKIN_MAX_INFLUENCES:
            raise ValueError('SkinWeights.from_dense: a row has %d non-zero weights, at most %d' % (K, _lib.SKIN_MAX_INFLUENCES))
        if J == 0:
            if V:
                raise ValueError('SkinWeights.from_dense: %d vertices and no bone' % V)
            return cls(torch.zeros(0, 1, dtype=torch.int32, device=weights.device), weights.new_zeros(0, 1), 0, chunk)
        # a stable sort brings the non-zero entries of a row to the front, in order of bone
        order = torch.argsort((~nonzero).to(torch.int32), dim=1, stable=True)[:, :K]
        kept = torch.gather(nonzero, 1, order)
        w = torch.where(kept, torch.gather(weights, 1, order), torch.zeros((), dtype=weights.dtype, device=weights.device))
        return cls(torch.where(kept, order, torch.zeros_like(order)).to(torch.int32), w, J, chunk)

    def dense(self, weights=None):
        """The [V, J] matrix of the weights (of `weights` [V, K] instead, if given): slots naming one bone add up."""
        w = self.bone_weights if weights is None else weights
        out = torch.zeros(self.num_vertices, self.num_bones, dtype=w.dtype, device=w.device)
        return out.scatter_add(1, self.bone_indices.long().to(w.device), w)


class _SkinVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, transforms, weights, skin, meta):
        lib = _lib.load()
        B, V, C, batched = meta
        dev = vertices.device
        posed = torch.empty(((B, V, 3) if batched else (V, 3)), dtype=torch.float32, device=dev)
        if B * V:
            _stage.call(lib.dirt_skin_forward, dev, *_operands(vertices, transforms, weights, skin), posed.data_ptr(), B, V, skin.influences,
                        skin.num_bones, 0)
        ctx.save_for_backward(vertices, transforms, weights)
        ctx.skin, ctx.meta = skin, meta
        return posed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_posed):
        lib = _lib.load()
        vertices, transforms, weights = ctx.saved_tensors
        skin = ctx.skin
        B, V, C, batched = ctx.meta
        dev = vertices.device
        want = ctx.needs_input_grad[:3]
        grads = _stage.grad_outputs((vertices, transforms, weights), want, not B * V)
        if not B * V:
            return tuple(grads) + (None, None)
        g = grad_posed.to(torch.float32).contiguous()
        nbytes = lib.dirt_skin_scratch_bytes(B, skin.num_chunks) if want[1] else 0
        _stage.call(lib.dirt_skin_backward, dev, *_operands(vertices, transforms, weights, skin), skin.entries.data_ptr() or None,
                    skin.chunk_table.data_ptr() or None, skin.chunk_offsets.data_ptr(), g.data_ptr(),
                    *(t.data_ptr() if t is not None else None for t in grads), _stage.ptr(_stage.scratch(dev, nbytes)), nbytes,
                    B, V, skin.influences, skin.num_bones, skin.num_chunks, 0)
        return tuple(grads) + (None, None)


def _operands(vertices, transforms, weights, skin):
    """the operands as the C ABI takes them: a shared operand has a scene count of 1"""
    return (vertices.data_ptr(), int(vertices.shape[-1]), 1 if vertices.dim() == 2 else int(vertices.shape[0]), skin.bone_indices.data_ptr(),
            weights.data_ptr(), transforms.data_ptr(), 1 if transforms.dim() == 3 else int(transforms.shape[0]))


def _check_arguments(vertices, skin, bone_transforms, weights):
    """Everything `skin_vertices` refuses with a ValueError, from shapes, dtypes and devices alone (no device work): ->
    (B, V, C, batched)"""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() not in (2, 3) or vertices.shape[-1] not in (3, 4):
        raise ValueError('skin_vertices expects vertices [V, 3|4] or [B, V, 3|4], got %s' % (tuple(getattr(vertices, 'shape', ())),))
    if vertices.dtype != torch.float32:
        raise ValueError('skin_vertices expects float32 vertices, got %s' % vertices.dtype)
    if not isinstance(skin, SkinWeights):
        raise ValueError('skin_vertices expects a SkinWeights (build it once per mesh), got %r' % type(skin).__name__)
    V, C = int(vertices.shape[-2]), int(vertices.shape[-1])
    if V != skin.num_vertices:
        raise ValueError('skin_vertices: %d vertices, the SkinWeights was built for %d' % (V, skin.num_vertices))
    _stage.check_index_device('skin_vertices', 'SkinWeights', 'skin', skin, 'vertices', vertices)
    _stage.check_operand('bone_transforms', bone_transforms, (skin.num_bones, 4, 4), vertices, 'vertices')
    B, batched = _stage.scene_count('skin_vertices', ('vertices', vertices, 3), ('bone_transforms', bone_transforms, 4))
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (V, skin.influences):   # (never per scene: no [B, ..] form)
            raise ValueError('weights must have shape [%d, %d], got %s' % (V, skin.influences, tuple(getattr(weights, 'shape', ())),))
        _stage.check_float32('weights', weights, vertices, 'vertices')
    return B, V, C, batched


def skin_vertices(vertices, skin, bone_transforms, weights=None):
    """Linear-blend skinning in one kernel, differentiably.  -> posed [.., V, 3]

    vertices: float32 [V, 3|4] (one rest mesh for every scene) or [B, V, 3|4] (per-scene vertices: blend shapes applied
        upstream) on the GPU; with three components w = 1 is appended.
    skin: the mesh's `SkinWeights`, on the same device.
    bone_transforms: float32 [J, 4, 4] or [B, J, 4, 4], in the row-vector convention of `dirt_amd.matrices` (v @ T,
        translation in row 3); GPU tensors, never read on the host.  `dirt_amd.kinematics.pose_skeleton` computes them from
        joint rotations (the forward kinematics of a skeleton, fused).
    weights: float32 [V, K] that replaces skin.bone_weights for this call and may require a gradient (learned weights).
    The output is batched if either input is.  Per scene
        M[v] = sum over k in slot order of w[v, k] * T[idx[v, k]],     posed[v] = (v4 @ M[v])[:3]
    in float32; column 3 of the transforms is never read and its gradient is written as zero.  Gradients (to all
    components of the vertices, to the transforms and to `weights`) are those of torch's autograd for this composition;
    an operand shared by the scenes receives the sum over the scenes.  No atomics: the same bits on every run.  Nothing
    in a call synchronises with the host."""
    meta = _check_arguments(vertices, skin, bone_transforms, weights)
    _stage.require_gpu(vertices, 'dirt_amd.skinning.skin_vertices')
    w = skin.bone_weights if weights is None else weights.contiguous()
    return _SkinVertices.apply(vertices.contiguous(), bone_transforms.contiguous(), w, skin, meta)
