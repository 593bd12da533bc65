"""The vertex stage in front of the rasteriser, fused: object-space vertices -> clip-space vertices, world positions and
world normals (what every sample of the reference computes with two matrix products and `lighting.vertex_normals`:
samples/deferred.py:40-51, samples/simple.py:45-56, samples/textured.py:97-108) as one HIP kernel forward and two or
three backward (dirt_geometry.hip; specification in DESIGN.md §7c).

    topology = MeshTopology(faces, num_vertices)          # once per mesh: the inverted index the kernels walk
    for it in range(n):
        clip, world, normals = vertex_stage(vertices, topology, model, view_projection)
        pixels = dirt_amd.rasterise_deferred(vertices=clip, faces=topology.faces, ...)

The scatter of `lighting.vertex_normals` (three `index_add`s, float atomics on a GPU) is a gather over the topology's
inverted index here: no atomics, one launch, and the same bits on every run.
"""
import torch

from . import _lib
from . import _stage

_WANT = ('clip', 'world', 'normals')
# Lists of more than this many entries are summed by a whole wave instead of their vertex's lane; None: the library's
# default (_lib.GEOM_LONG_LIST_DEFAULT, chosen by measurement: DESIGN.md §7c).  For measurements (tools/bench_geometry.py).
LONG_LIST = None


class MeshTopology(_stage.StageIndex):
    """The faces of a mesh and their inverted index, built once (topology is constant across a fitting loop).

    faces: int32 / int64 [F, 3] on any device; num_vertices: V.  Indices outside [0, V), another shape or dtype raise
    ValueError (this reads one value back from the device; `vertex_stage` never does).
    Attributes, all int32 on the device of `faces`:
        faces [F, 3]; offsets [V + 1]; entries [3 F]: the entries of vertex v are entries[offsets[v]:offsets[v + 1]], each
        3 * face + corner, ordered by face, then corner.  A vertex no face names has an empty list; a face that names a
        vertex twice contributes two entries.
    """

    def __init__(self, faces, num_vertices):
        if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError('MeshTopology expects faces [F, 3], got %s' % (tuple(getattr(faces, 'shape', ())),))
        if faces.dtype not in (torch.int32, torch.int64):
            raise ValueError('MeshTopology expects int32 or int64 faces, got %s' % faces.dtype)   # dirt/lighting.py:15-17
        if isinstance(num_vertices, bool) or not isinstance(num_vertices, int) or num_vertices < 0:
            raise ValueError('MeshTopology expects num_vertices >= 0, got %r' % (num_vertices,))
        if num_vertices > _lib.GEOM_MAX_VERTICES or faces.shape[0] > _lib.GEOM_MAX_FACES:
            raise ValueError('MeshTopology: at most %d vertices and %d faces' % (_lib.GEOM_MAX_VERTICES, _lib.GEOM_MAX_FACES))
        flat = faces.reshape(-1).long()   # position 3 * face + corner
        _stage.check_index_range(flat, num_vertices, 'MeshTopology: faces name vertices %d..%d, outside [0, %d)')
        # a stable sort of the positions by vertex keeps them in order of face, then corner
        entries = torch.argsort(flat, stable=True).to(torch.int32)
        offsets = _stage.sort_offsets(flat, num_vertices)
        self.num_vertices, self.num_faces = num_vertices, int(faces.shape[0])
        self.faces, self.offsets, self.entries = faces.to(torch.int32).contiguous(), offsets.to(torch.int32), entries.contiguous()

    _TENSORS = ('faces', 'offsets', 'entries')


class _VertexStage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, model, view_projection, topology, meta):
        lib = _lib.load()
        B, V, C, batched, want, flags = meta
        dev = vertices.device
        lead = (B, V) if batched else (V,)
        clip, world, normals = (torch.empty(lead + (w,), dtype=torch.float32, device=dev) if name in want else None
                                for name, w in (('clip', 4), ('world', 4), ('normals', 3)))
        if B * V:
            _stage.call(lib.dirt_geometry_forward, dev, vertices.data_ptr(), C, *_index_pointers(topology),
                        *_matrix_arguments(model, view_projection), *(t.data_ptr() if t is not None else None for t in (clip, world, normals)),
                        B, V, topology.num_faces, flags)
        ctx.save_for_backward(vertices, model, view_projection)
        ctx.topology, ctx.meta = topology, meta
        return clip, world, normals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_clip, grad_world, grad_normals):
        lib = _lib.load()
        vertices, model, view_projection = ctx.saved_tensors
        topology = ctx.topology
        B, V, C, batched, want, flags = ctx.meta
        dev = vertices.device
        grads = _stage.grad_outputs((vertices, model, view_projection), ctx.needs_input_grad[:3], not B * V)
        if not B * V:
            return tuple(grads) + (None, None)
        incoming = _stage.float32_contiguous(grad_clip, grad_world, grad_normals)
        nbytes = lib.dirt_geometry_scratch_bytes(B, V, topology.num_faces)
        _stage.call(lib.dirt_geometry_backward, dev, vertices.data_ptr(), C, *_index_pointers(topology),
                    *_matrix_arguments(model, view_projection), *(g.data_ptr() if g is not None else None for g in incoming),
                    *(g.data_ptr() if g is not None else None for g in grads), _stage.ptr(_stage.scratch(dev, nbytes)), nbytes,
                    B, V, topology.num_faces, flags)
        return tuple(grads) + (None, None)


def _index_pointers(topology):
    # (an empty tensor's data_ptr() is 0: NULL, which the library accepts for a mesh without faces)
    return tuple(t.data_ptr() or None for t in (topology.faces, topology.offsets, topology.entries))


def _matrix_arguments(model, view_projection):
    """(pointer, scene count) of each matrix as the C ABI takes them: ([4, 4] -> 1, [B, 4, 4] -> B, None -> NULL, 0)"""
    out = []
    for m in (model, view_projection):
        out += [m.data_ptr(), 1 if m.dim() == 2 else int(m.shape[0])] if m is not None else [None, 0]
    return out


def _check_arguments(vertices, topology, model, view_projection, pre_split, want):
    """Everything `vertex_stage` refuses with a ValueError, from shapes, dtypes and devices alone (no device work): ->
    (B, V, C, batched, the wanted outputs in canonical order, flags)"""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() not in (2, 3) or vertices.shape[-1] not in (3, 4):
        raise ValueError('vertex_stage expects vertices [V, 3|4] or [B, V, 3|4], got %s' % (tuple(getattr(vertices, 'shape', ())),))
    if vertices.dtype != torch.float32:
        raise ValueError('vertex_stage expects float32 vertices, got %s' % vertices.dtype)
    if not isinstance(topology, MeshTopology):
        raise ValueError('vertex_stage expects a MeshTopology (build it once per mesh), got %r' % type(topology).__name__)
    V, C = int(vertices.shape[-2]), int(vertices.shape[-1])
    if V != topology.num_vertices:
        raise ValueError('vertex_stage: %d vertices, the topology was built for %d' % (V, topology.num_vertices))
    B, batched = _stage.scene_count('vertex_stage', ('vertices', vertices, 3))
    _stage.check_index_device('vertex_stage', 'topology', 'topology', topology, 'vertices', vertices)
    for name, m in (('model', model), ('view_projection', view_projection)):
        if m is None:
            continue
        shapes = [(4, 4), (B, 4, 4)] if batched else [(4, 4)]   # (a matrix per scene only with vertices per scene, and then B is known)
        if not isinstance(m, torch.Tensor) or tuple(m.shape) not in shapes:
            raise ValueError('%s must have shape %s, got %s' % (name, ' or '.join(str(list(s)) for s in shapes), tuple(getattr(m, 'shape', ()))))
        _stage.check_float32(name, m, vertices, 'vertices')
    if isinstance(want, str) or any(w not in _WANT for w in want):
        raise ValueError('want must be a sequence of %s, got %r' % (_WANT, want))
    want = tuple(w for w in _WANT if w in want)
    if 'clip' in want and view_projection is None:
        want = tuple(w for w in want if w != 'clip')   # clip is None without a view_projection
    long_list = (int(LONG_LIST) << _lib.GEOM_LONG_LIST_SHIFT) & _lib.GEOM_LONG_LIST_MASK if LONG_LIST else 0
    return B, V, C, batched, want, (_lib.GEOM_PRE_SPLIT if pre_split else 0) | long_list


def vertex_stage(vertices, topology, model=None, view_projection=None, *, pre_split=False, want=_WANT):
    """Transforms and vertex normals in one kernel (samples/deferred.py:40-51), differentiably.  -> (clip, world, normals)

    vertices: float32 [V, 3|4] or [B, V, 3|4] on the GPU; with three components w = 1 is appended.
    topology: the mesh's `MeshTopology`, on the same device.
    model, view_projection: [4, 4], or [B, 4, 4] with batched vertices, in the row-vector convention of
        `dirt_amd.matrices` (v @ M); GPU tensors, differentiable, never read on the host.
    world4 = v4 @ model (v4 itself without a model); clip = world4 @ view_projection (None without one);
    normals = lighting.vertex_normals(world4, faces), or lighting.vertex_normals_pre_split(world4, faces) with
    pre_split=True, the reference's two 1e-12s included (dirt/lighting.py:21-28,31-89,97-129).
    Returns clip [.., V, 4], world [.., V, 4], normals [.., V, 3]; outputs not named in `want` are None and are neither
    computed nor written.  Values are this float32 composition; gradients (to all components of the vertices and to both
    matrices) are those of torch's autograd for it: the norm of a zero vector has gradient 0, so a zero-area face passes
    d n / 1e-12 to its cross product and nothing through the norm.  Nothing in a call synchronises with the host."""
    meta = _check_arguments(vertices, topology, model, view_projection, pre_split, want)
    _stage.require_gpu(vertices, 'dirt_amd.geometry.vertex_stage')
    v = vertices.contiguous()
    model, view_projection = (m.contiguous() if m is not None else None for m in (model, view_projection))
    return _VertexStage.apply(v, model, view_projection, topology, meta)


def vertex_normals(vertices, topology, pre_split=False):
    """`lighting.vertex_normals(vertices, faces)` (or `vertex_normals_pre_split` with pre_split=True) alone, in one kernel:
    [.., V, 3|4] -> [.., V, 3] (dirt/lighting.py:31-89,97-129)."""
    return vertex_stage(vertices, topology, pre_split=pre_split, want=('normals',))[2]


# ---- per-vertex tangent frames (dirt_tangent.hip)

class _VertexTangents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, normals, uvs, topology, meta):
        lib = _lib.load()
        B, V, C, batched = meta
        dev = vertices.device
        tangents = torch.empty(((B, V) if batched else (V,)) + (4,), dtype=torch.float32, device=dev)
        if B * V:
            _stage.call(lib.dirt_tangent_forward, dev, vertices.data_ptr(), C, normals.data_ptr(), uvs.data_ptr(), *_index_pointers(topology),
                        tangents.data_ptr(), B, V, topology.num_faces)
        ctx.save_for_backward(vertices, normals, uvs)
        ctx.topology, ctx.meta = topology, meta
        return tangents

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_tangents):
        lib = _lib.load()
        vertices, normals, uvs = ctx.saved_tensors
        topology = ctx.topology
        B, V, C, batched = ctx.meta
        dev = vertices.device
        grads = _stage.grad_outputs((vertices, normals), ctx.needs_input_grad[:2], not B * V)
        if not B * V:
            return tuple(grads) + (None, None, None)
        incoming, = _stage.float32_contiguous(grad_tangents)
        nbytes = lib.dirt_tangent_scratch_bytes(B, V, topology.num_faces) if grads[0] is not None else 0
        _stage.call(lib.dirt_tangent_backward, dev, vertices.data_ptr(), C, normals.data_ptr(), uvs.data_ptr(), *_index_pointers(topology),
                    incoming.data_ptr(), *(_stage.ptr(g) for g in grads), _stage.ptr(_stage.scratch(dev, nbytes)), nbytes,
                    B, V, topology.num_faces)
        return tuple(grads) + (None, None, None)


def _check_tangent_arguments(vertices, normals, uvs, topology):
    """Everything `vertex_tangents` refuses with a ValueError, from shapes, dtypes and devices alone (no device work): ->
    (B, V, C, batched)"""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() not in (2, 3) or vertices.shape[-1] not in (3, 4):
        raise ValueError('vertex_tangents expects vertices [V, 3|4] or [B, V, 3|4], got %s' % (tuple(getattr(vertices, 'shape', ())),))
    if vertices.dtype != torch.float32:
        raise ValueError('vertex_tangents expects float32 vertices, got %s' % vertices.dtype)
    if not isinstance(topology, MeshTopology):
        raise ValueError('vertex_tangents expects a MeshTopology (build it once per mesh), got %r' % type(topology).__name__)
    V, C = int(vertices.shape[-2]), int(vertices.shape[-1])
    if V != topology.num_vertices:
        raise ValueError('vertex_tangents: %d vertices, the topology was built for %d' % (V, topology.num_vertices))
    want = tuple(vertices.shape[:-1]) + (3,)
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != want:
        raise ValueError('normals must have shape %s (the vertices\' %s with 3 components), got %s'
                         % (list(want), list(vertices.shape), list(getattr(normals, 'shape', ()))))
    _stage.check_float32('normals', normals, vertices, 'vertices')
    if not isinstance(uvs, torch.Tensor) or tuple(uvs.shape) != (V, 2):
        raise ValueError('uvs must have shape [%d, 2] (one pair per vertex, shared by the scenes), got %s' % (V, list(getattr(uvs, 'shape', ()))))
    _stage.check_float32('uvs', uvs, vertices, 'vertices')
    B, batched = _stage.scene_count('vertex_tangents', ('vertices', vertices, 3))
    _stage.check_index_device('vertex_tangents', 'topology', 'topology', topology, 'vertices', vertices)
    return B, V, C, batched


def vertex_tangents(vertices, normals, uvs, topology):
    """`lighting.vertex_tangents(vertices, normals, uvs, faces)` in one kernel, differentiably: the per-vertex tangent frames
    of tangent-space normal mapping, -> [.., V, 4] (the unit tangent, orthogonal to the normal, along increasing u; the
    handedness -1 / +1 of the bitangent).  Interpolated over the mesh next to the normals, they are what
    `shading.perturb_normals` takes.

    vertices: float32 [V, 3|4] or [B, V, 3|4] on the GPU (only x, y, z are used); normals: [.., V, 3] with the same lead,
        taken as given (unit, as `vertex_stage` returns them); uvs: float32 [V, 2] on the same device, shared by the scenes,
        constant; topology: the mesh's `MeshTopology`.
    A vertex no face names, or whose faces are all degenerate in uv, gets (0, 0, 0, 1).  Gradients go to the vertices (a
    fourth component gets zeros) and to the normals; the handedness is a sign and carries none.  The scatter of the torch
    form (six `index_add`s) is a gather over the topology's inverted index, forward and backward: no atomics, the same bits
    on every run, and nothing in a call synchronises with the host."""
    meta = _check_tangent_arguments(vertices, normals, uvs, topology)
    _stage.require_gpu(vertices, 'dirt_amd.geometry.vertex_tangents')
    return _VertexTangents.apply(vertices.contiguous(), normals.contiguous(), uvs.detach().contiguous(), topology, meta)
