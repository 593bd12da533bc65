"""Blend shapes at the head of the fused chain: a template mesh, shape coefficients and a table of directions -> the
rest-pose vertices `skin_vertices` takes and the rest-pose joint positions `pose_skeleton` takes.  The reference's samples
render one fixed mesh (samples/deferred.py:40-41 moves it with one matrix); a body, hand or face model (SMPL, MANO, SMPL-X,
FLAME) makes its rest mesh as template + sum of coefficient x direction -- identity shape, expression and pose correctives
alike -- and regresses its joints from the shaped mesh.  One HIP kernel forward, one to three backward (dirt_blend.hip;
specification in DESIGN.md §7f).

    shapes = BlendShapes(directions, joint_regressor, joint_shapes=10)      # once per model: the packed table, the regressor's two indices
    for it in range(n):
        features = pose_corrective_features(rotations)                      # SMPL's pose correctives: 9 (J - 1) more coefficients
        rest, joints = blend_shapes(template, torch.cat([betas, features], -1), shapes)
        transforms, _ = dirt_amd.pose_skeleton(rotations, joints, skeleton)
        posed = dirt_amd.skin_vertices(rest, skin, transforms)

In torch this is two matmuls over the [K, 3 V] table, two adds and a dense [J, V] joint regression that is more than 99 %
zeros, with sums whose order the BLAS library chooses; here every sum has a fixed order: the same bits on every run.
"""
import torch

from . import _lib
from . import _stage
from . import matrices
from ._stage import ptr as _ptr


class BlendShapes(_stage.StageIndex):
    """The direction table of a model, its joint regressor and what the kernels read of them, built once.

    directions: float32 [K, V, 3], 0 <= K <= 4096, V <= 2^26, on any one device.
    joint_regressor: float32 dense [J, V] in SMPL's style (joints = regressor @ vertices), J <= 256, on the same device; None:
        no joints (J = 0).  Its non-zeros number at most 2^30.
    joint_shapes: Ks, 0 <= Ks <= K (default K): only the first Ks directions move the joints -- SMPL's rule: the joints are
        regressed from the shaped mesh, before the pose correctives.
    Anything else raises ValueError.  All of this is CONSTANT: `blend_shapes` sends no gradient to the directions or the
    regressor, and a tensor given here that requires one is detached.
    Attributes (on the device of `directions`; int32 unless noted):
        packed [K, stride] float32: row k is directions[k] as 3 V floats, then zeros; stride = 3 V rounded up to a multiple of
        4, so that every row starts 16-byte aligned (a raw [K, 3 V] row starts 4-byte aligned whenever 3 V is no multiple of
        4) and a lane reads 16 bytes;
        the regressor by joint (CSR): row_offsets [J + 1], row_vertices, row_weights float32 -- its non-zeros ordered by joint,
        then vertex, those of joint j at row_offsets[j]:row_offsets[j + 1];
        the regressor by vertex (CSC), the inverted index the template's gradient gathers over: column_offsets [V + 1],
        column_joints, column_weights float32 -- the non-zeros ordered by vertex, then joint;
        joint_directions [Ks, J, 3] float32: regressor @ directions[k], computed once in float64 and rounded.
    """

    def __init__(self, directions, joint_regressor=None, joint_shapes=None):
        if not isinstance(directions, torch.Tensor) or directions.dim() != 3 or directions.shape[2] != 3:
            raise ValueError('BlendShapes expects directions [K, V, 3], got %s' % (tuple(getattr(directions, 'shape', ())),))
        if directions.dtype != torch.float32:
            raise ValueError('BlendShapes expects float32 directions, got %s' % directions.dtype)
        K, V = int(directions.shape[0]), int(directions.shape[1])
        if K > _lib.BLEND_MAX_SHAPES or V > _lib.BLEND_MAX_VERTICES:
            raise ValueError('BlendShapes: %d shapes of %d vertices, at most %d shapes and %d vertices' % (K, V, _lib.BLEND_MAX_SHAPES, _lib.BLEND_MAX_VERTICES))
        dev = directions.device
        R = joint_regressor
        if R is None:
            R = torch.zeros(0, V, dtype=torch.float32, device=dev)
        if not isinstance(R, torch.Tensor) or R.dim() != 2 or int(R.shape[1]) != V:
            raise ValueError('BlendShapes expects a joint_regressor [J, %d], got %s' % (V, tuple(getattr(R, 'shape', ())),))
        if R.dtype != torch.float32:
            raise ValueError('BlendShapes expects a float32 joint_regressor, got %s' % R.dtype)
        if R.device != dev:
            raise ValueError('BlendShapes: joint_regressor is on %s, directions on %s' % (R.device, dev))
        J = int(R.shape[0])
        if J > _lib.BLEND_MAX_JOINTS:
            raise ValueError('BlendShapes: %d joints, at most %d' % (J, _lib.BLEND_MAX_JOINTS))
        Ks = K if joint_shapes is None else joint_shapes
        if isinstance(Ks, bool) or not isinstance(Ks, int) or not 0 <= Ks <= K:
            raise ValueError('BlendShapes expects 0 <= joint_shapes <= K = %d, got %r' % (K, joint_shapes))
        directions, R = directions.detach(), R.detach()
        E = 3 * V
        stride = (E + 3) // 4 * 4
        packed = torch.zeros(K, stride, dtype=torch.float32, device=dev)
        packed[:, :E] = directions.reshape(K, E)
        # torch.nonzero lists the non-zeros in row-major order: of R by joint, then vertex; of its transpose by vertex, then joint
        by_joint, by_vertex = torch.nonzero(R), torch.nonzero(R.t())
        if by_joint.shape[0] > _lib.BLEND_MAX_ENTRIES:
            raise ValueError('BlendShapes: the joint_regressor has %d non-zeros, at most %d' % (by_joint.shape[0], _lib.BLEND_MAX_ENTRIES))
        row_offsets, column_offsets = _stage.sort_offsets(by_joint[:, 0], J), _stage.sort_offsets(by_vertex[:, 0], V)
        self.num_shapes, self.num_vertices, self.num_joints, self.joint_shapes, self.stride = K, V, J, Ks, stride
        self.packed = packed
        self.row_offsets, self.row_vertices = row_offsets.to(torch.int32), by_joint[:, 1].to(torch.int32).contiguous()
        self.row_weights = R[by_joint[:, 0], by_joint[:, 1]].contiguous()
        self.column_offsets, self.column_joints = column_offsets.to(torch.int32), by_vertex[:, 1].to(torch.int32).contiguous()
        self.column_weights = R[by_vertex[:, 1], by_vertex[:, 0]].contiguous()
        self.joint_directions = torch.einsum('jv,kvc->kjc', R.double(), directions[:Ks].double()).to(torch.float32).contiguous()

    _TENSORS = ('packed', 'row_offsets', 'row_vertices', 'row_weights', 'column_offsets', 'column_joints', 'column_weights', 'joint_directions')

    def directions(self):
        """The [K, V, 3] table, out of the packed copy."""
        return self.packed[:, :3 * self.num_vertices].reshape(self.num_shapes, self.num_vertices, 3)

    def dense_regressor(self):
        """The dense [J, V] regressor, out of the non-zeros ordered by joint."""
        out = torch.zeros(self.num_joints, self.num_vertices, dtype=torch.float32, device=self.device)
        joint = torch.repeat_interleave(torch.arange(self.num_joints, device=self.device), torch.diff(self.row_offsets.long()))
        out[joint, self.row_vertices.long()] = self.row_weights
        return out


class _BlendShapes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, template, coefficients, shapes, meta):
        lib = _lib.load()
        B, V, K, J, batched = meta
        dev = template.device
        lead = (B,) if batched else ()
        vertices = torch.empty(lead + (V, 3), dtype=torch.float32, device=dev)
        joints = torch.empty(lead + (J, 3), dtype=torch.float32, device=dev)
        if B * V:
            _stage.call(lib.dirt_blend_forward, dev, _ptr(template), 1 if template.dim() == 2 else B, _ptr(coefficients),
                        1 if coefficients.dim() == 1 else B, _ptr(shapes.packed), shapes.stride, shapes.row_offsets.data_ptr(),
                        _ptr(shapes.row_vertices), _ptr(shapes.row_weights), _ptr(shapes.joint_directions), vertices.data_ptr(), _ptr(joints),
                        B, V, K, shapes.joint_shapes, J, 0)
        else:
            joints.zero_()   # no vertex: every sum is empty
        ctx.shapes, ctx.meta = shapes, meta
        ctx.operand_shapes = (template.shape, coefficients.shape)
        ctx.set_materialize_grads(False)   # an output nobody used arrives as None and contributes nothing
        return vertices, joints

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_vertices, grad_joints):
        lib = _lib.load()
        shapes = ctx.shapes
        B, V, K, J, batched = ctx.meta
        dev = shapes.device
        want = ctx.needs_input_grad[:2]
        # (what _stage.grad_outputs makes, from the shapes: no operand is kept for the backward)
        grads = [torch.empty(s, dtype=torch.float32, device=dev) if on else None for s, on in zip(ctx.operand_shapes, want)]
        if not B * V:
            return tuple(g.zero_() if g is not None else None for g in grads) + (None, None)
        gv, gj = _stage.float32_contiguous(grad_vertices, grad_joints)
        nbytes = lib.dirt_blend_scratch_bytes(B, V, K) if want[1] and K else 0
        _stage.call(lib.dirt_blend_backward, dev, 1 if len(ctx.operand_shapes[0]) == 2 else B, 1 if len(ctx.operand_shapes[1]) == 1 else B,
                    _ptr(shapes.packed), shapes.stride, shapes.column_offsets.data_ptr(), _ptr(shapes.column_joints), _ptr(shapes.column_weights),
                    _ptr(shapes.joint_directions), _ptr(gv), _ptr(gj), _ptr(grads[0]), _ptr(grads[1]), _ptr(_stage.scratch(dev, nbytes)), nbytes,
                    B, V, K, shapes.joint_shapes, J, 0)
        return tuple(grads) + (None, None)


def _check_arguments(template, coefficients, shapes):
    """Everything `blend_shapes` refuses with a ValueError, from shapes, dtypes and devices alone (no device work): ->
    (B, V, K, J, batched)"""
    if not isinstance(shapes, BlendShapes):
        raise ValueError('blend_shapes expects a BlendShapes (build it once per model), got %r' % type(shapes).__name__)
    V, K = shapes.num_vertices, shapes.num_shapes
    _stage.check_operand('template', template, (V, 3))
    _stage.check_operand('coefficients', coefficients, (K,), template, 'template')
    _stage.check_index_device('blend_shapes', 'BlendShapes', 'shapes', shapes, 'template', template)
    B, batched = _stage.scene_count('blend_shapes', ('template', template, 3), ('coefficients', coefficients, 2))
    return B, V, K, shapes.num_joints, batched


def blend_shapes(template, coefficients, shapes):
    """The rest mesh and rest joints of a blend-shape model in one kernel, differentiably.  -> (vertices [.., V, 3], joints [.., J, 3])

    template: float32 [V, 3] (one for every scene) or [B, V, 3] on the GPU.
    coefficients: float32 [K] or [B, K]: identity shape, expression, pose correctives (`pose_corrective_features`), in the
        order of the table's directions.
    shapes: the model's `BlendShapes`, on the same device.  GPU tensors, never read on the host.
    The two combine freely; the outputs are batched if either input is (B <= 65535); joints is [.., 0, 3] without a regressor.
    Per scene, in float32,
        vertices[v] = template[v] + sum over k < K of c[k] * directions[k, v]
        joints[j]   = sum over the regressor's non-zeros (j, v), by v, of w[j, v] * template[v]
                    + sum over k < Ks of c[k] * joint_directions[k, j]
    with the order of every sum fixed by the kernel: the same bits on every run.  Gradients go to the
    template and the coefficients, from either output, and are those of torch's autograd for this composition; an operand
    shared by the scenes receives the sum over the scenes.  The directions and the regressor are constants: they receive no
    gradient.  No atomics.  Nothing in a call synchronises with the host."""
    meta = _check_arguments(template, coefficients, shapes)
    _stage.require_gpu(template, 'dirt_amd.blendshapes.blend_shapes')
    return _BlendShapes.apply(template.contiguous(), coefficients.contiguous(), shapes, meta)


def pose_corrective_features(rotations):
    """SMPL's pose-corrective coefficients (a torch helper, no kernel): angle-axis rotations [.., J, 3] -> [.., 9 (J - 1)], the
    flattened R_j - I of the non-root joints j = 1 .. J - 1, to be concatenated behind the shape coefficients.

    R_j = matrices.rodrigues(rotations[j], three_by_three=True) is flattened row-major AS RETURNED, indexed [in, out] -- no
    transpose: numerically it is the matrix cv2.Rodrigues gives for the same vector (a turn by a about z has R[0, 1] = -sin a),
    the one SMPL's `posedirs` were learned against.  (Under the row-vector convention of `dirt_amd.matrices`, v @ R, that is the
    transpose of the matrix that would turn a column vector the same way.)"""
    if not isinstance(rotations, torch.Tensor) or rotations.dim() < 2 or rotations.shape[-1] != 3 or rotations.shape[-2] < 1:
        raise ValueError('pose_corrective_features expects rotations [.., J, 3] with J >= 1, got %s' % (tuple(getattr(rotations, 'shape', ())),))
    R = matrices.rodrigues(rotations[..., 1:, :], three_by_three=True)
    eye = torch.eye(3, dtype=R.dtype, device=R.device)
    return (R - eye).reshape(rotations.shape[:-2] + (9 * (int(rotations.shape[-2]) - 1),))
