"""Forward kinematics in front of the skinning stage, fused: the angle-axis rotations and rest-pose joint positions of a
skeleton -> the bone transforms `skin_vertices` takes, and the posed joint positions.  The reference's samples turn a mesh
with one `matrices.rodrigues` / `compose` (samples/deferred.py:40-41); an articulated body (SMPL: 24 joints, MANO: 16,
SMPL-X: 55) composes one per joint along its tree, every joint waiting for its parent -- several hundred tiny launches in
torch.  One HIP kernel forward, one or two backward (dirt_kinematics.hip; specification in DESIGN.md §7e).

    skeleton = Skeleton(parents)                                        # once per rig: levels and the inverted index of `parents`
    for it in range(n):
        transforms, posed_joints = pose_skeleton(rotations, joints, skeleton)
        posed = dirt_amd.skin_vertices(rest, skin, transforms)

The scatter of a child's gradient into its parent is a gather over the inverted index here: no atomics, and the same bits
on every run.
"""
import torch

from . import _lib
from . import _stage
from ._stage import ptr as _ptr


class Skeleton(_stage.StageIndex):
    """The tree (or forest) of a rig and the index the kernels walk, built once.

    parents: a sequence of ints or an integer tensor [J], 0 <= J <= 256.  parents[j] == -1 marks a root (several are
    allowed); otherwise 0 <= parents[j] < j: parents come before their children, as SMPL, MANO and SMPL-X order them.
    Anything else raises ValueError (this reads `parents` on the host; `pose_skeleton` never does).  device: where the
    tensors go (default: that of a `parents` tensor, else the CPU).
    Attributes (int32, on one device):
        parents [J];
        order [J]: the joints by depth, then index; level_offsets [D + 1]: level d -- the joints of depth d, level 0 the
        roots -- is order[level_offsets[d]:level_offsets[d + 1]];
        child_entries [J - roots]: the non-root joints ordered by parent, then index; child_offsets [J + 1]: the children
        of joint j are child_entries[child_offsets[j]:child_offsets[j + 1]].
    """

    def __init__(self, parents, device=None):
        J_MAX = _lib.KINEMATICS_MAX_JOINTS
        if isinstance(parents, torch.Tensor):
            if parents.dim() != 1 or parents.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
                raise ValueError('Skeleton expects an integer tensor [J] of parents, got %s %s' % (parents.dtype, tuple(parents.shape)))
            device = parents.device if device is None else device
            host = parents.detach().cpu().tolist()
        else:
            try:
                host = list(parents)
            except TypeError:
                raise ValueError('Skeleton expects a sequence or an integer tensor [J] of parents, got %r' % type(parents).__name__)
            if any(isinstance(x, bool) or not isinstance(x, int) for x in host):
                raise ValueError('Skeleton expects integer parents, got %r' % (host,))
        J = len(host)
        if J > J_MAX:
            raise ValueError('Skeleton: %d joints, at most %d' % (J, J_MAX))
        depth = []
        for j, q in enumerate(host):
            if not -1 <= q < j:
                raise ValueError('Skeleton: parents[%d] = %d; -1 marks a root, every other joint names a parent before it (0 <= parent < %d)' % (j, q, j))
            depth.append(0 if q < 0 else depth[q] + 1)
        dev = torch.device('cpu' if device is None else device)
        par = torch.tensor(host, dtype=torch.int64, device=dev).reshape(J)
        dep = torch.tensor(depth, dtype=torch.int64, device=dev).reshape(J)
        levels = max(depth) + 1 if J else 0
        # stable sorts keep the joints of a level, and the children of a parent, in order of index
        order = torch.argsort(dep, stable=True)
        level_offsets = _stage.sort_offsets(dep, levels)
        children = torch.nonzero(par >= 0)[:, 0]
        child_entries = children[torch.argsort(par[children], stable=True)]
        child_offsets = _stage.sort_offsets(par[children], J)
        self.num_joints, self.num_levels = J, levels
        self.parents, self.order, self.level_offsets = par.to(torch.int32), order.to(torch.int32).contiguous(), level_offsets.to(torch.int32)
        self.child_entries, self.child_offsets = child_entries.to(torch.int32).contiguous(), child_offsets.to(torch.int32)

    _TENSORS = ('parents', 'order', 'level_offsets', 'child_entries', 'child_offsets')


def _index_operands(skeleton):
    return (skeleton.parents.data_ptr(), skeleton.order.data_ptr(), skeleton.level_offsets.data_ptr(), skeleton.num_levels)


def _operands(rotations, joints):
    """the operands as the C ABI takes them: a shared operand has a scene count of 1"""
    return (rotations.data_ptr(), 1 if rotations.dim() == 2 else int(rotations.shape[0]),
            joints.data_ptr(), 1 if joints.dim() == 2 else int(joints.shape[0]))


class _PoseSkeleton(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotations, joints, skeleton, meta):
        lib = _lib.load()
        B, J, batched = meta
        dev = rotations.device
        lead = (B,) if batched else ()
        transforms = torch.empty(lead + (J, 4, 4), dtype=torch.float32, device=dev)
        posed_joints = torch.empty(lead + (J, 3), dtype=torch.float32, device=dev)
        if B * J:
            _stage.call(lib.dirt_kinematics_forward, dev, *_operands(rotations, joints), *_index_operands(skeleton), transforms.data_ptr(),
                        posed_joints.data_ptr(), B, J, 0)
        ctx.save_for_backward(rotations, joints)
        ctx.skeleton, ctx.meta = skeleton, meta
        ctx.set_materialize_grads(False)   # an output nobody used arrives as None and contributes nothing
        return transforms, posed_joints

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_transforms, grad_posed_joints):
        lib = _lib.load()
        rotations, joints = ctx.saved_tensors
        skeleton = ctx.skeleton
        B, J, batched = ctx.meta
        dev = rotations.device
        want = ctx.needs_input_grad[:2]
        grads = _stage.grad_outputs((rotations, joints), want, not B * J)
        if not B * J:
            return tuple(grads) + (None, None)
        incoming = _stage.float32_contiguous(grad_transforms, grad_posed_joints)
        shared = B > 1 and any(on and t.dim() == 2 for t, on in zip((rotations, joints), want))
        nbytes = lib.dirt_kinematics_scratch_bytes(B, J) if shared else 0
        _stage.call(lib.dirt_kinematics_backward, dev, *_operands(rotations, joints), *_index_operands(skeleton), _ptr(skeleton.child_entries),
                    skeleton.child_offsets.data_ptr(), *map(_ptr, incoming), *map(_ptr, grads), _ptr(_stage.scratch(dev, nbytes)), nbytes, B, J, 0)
        return tuple(grads) + (None, None)


def _check_arguments(rotations, joints, skeleton):
    """Everything `pose_skeleton` refuses with a ValueError, from shapes, dtypes and devices alone (no device work): ->
    (B, J, batched)"""
    if not isinstance(skeleton, Skeleton):
        raise ValueError('pose_skeleton expects a Skeleton (build it once per rig), got %r' % type(skeleton).__name__)
    J = skeleton.num_joints
    _stage.check_operand('rotations', rotations, (J, 3))
    _stage.check_operand('joints', joints, (J, 3), rotations, 'rotations')
    _stage.check_index_device('pose_skeleton', 'Skeleton', 'skeleton', skeleton, 'rotations', rotations)
    B, batched = _stage.scene_count('pose_skeleton', ('rotations', rotations, 3), ('joints', joints, 3))
    return B, J, batched


def pose_skeleton(rotations, joints, skeleton):
    """The forward kinematics of a skeleton in one kernel, differentiably.  -> (transforms [.., J, 4, 4], posed_joints [.., J, 3])

    rotations: float32 [J, 3] or [B, J, 3], angle-axis vectors as `matrices.rodrigues` takes them: joint j turns about its
        own position, in the frame of its parent.
    joints: float32 [J, 3] or [B, J, 3], the rest-pose joint positions (per scene where a body shape moves them).
    skeleton: the rig's `Skeleton`, on the same device.  GPU tensors, never read on the host.
    The outputs are batched if either input is.  Per scene, in float32 and the row-vector convention of `dirt_amd.matrices`,
        R[j]  = matrices.rodrigues(r[j], three_by_three=True)            tl[j] = p[j] - p[j] @ R[j]
        root:   S3[j] = R[j],                 t[j] = tl[j]
        else:   S3[j] = R[j] @ S3[parent],    t[j] = tl[j] @ S3[parent] + t[parent]
        transforms[j] = [[S3[j], 0], [t[j], 1]]                          posed_joints[j] = p[j] @ S3[j] + t[j]
    -- the composition translation(-p[j]) @ rodrigues(r[j]) @ translation(p[j]) @ transforms[parent] of
    examples/fit_pose_fused.py's loop, for a tree; `transforms` is what `skin_vertices` takes.  Global placement stays with
    `vertex_stage`'s `model` matrix.  Gradients (to the rotations and the joints, from either output; the one at a zero
    rotation vector included) are those of torch's autograd for this composition; an operand shared by the scenes receives
    the sum over the scenes.  No atomics: the same bits on every run.  Nothing in a call synchronises with the host."""
    meta = _check_arguments(rotations, joints, skeleton)
    _stage.require_gpu(rotations, 'dirt_amd.kinematics.pose_skeleton')
    return _PoseSkeleton.apply(rotations.contiguous(), joints.contiguous(), skeleton, meta)
