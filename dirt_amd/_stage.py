"""What the Python wrappers of the fused stages share (geometry, skinning, kinematics, blendshapes; of shading the call and
the backward plumbing; of the texture look-up the call, the pointers and the CPU refusal; of both the rule for rows read in place).  Private: the stages' own modules are the interface.
"""
import torch

from . import _lib
from . import rasterise_ops as _ops


class StageIndex:
    """The base of the built-once index objects: tensors, named in `_TENSORS`, and python scalars beside them."""
    _TENSORS = ()

    @property
    def device(self):
        return getattr(self, self._TENSORS[0]).device

    def to(self, device):
        """The same object with its tensors on `device` (nothing is rebuilt or checked again)."""
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(other, name, getattr(self, name).to(device))
        return other


def sort_offsets(keys, n):
    """The offsets of a counting sort: int64 keys in [0, n) -> int64 [n + 1]; sorted by key, those equal to k are at
    offsets[k]:offsets[k + 1]."""
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=keys.device)
    offsets[1:] = torch.cumsum(torch.bincount(keys, minlength=n), 0)
    return offsets


def check_index_range(flat, n, text):
    """Refuses int64 indices outside [0, n) with text % (lowest, highest, n); reads one value back from the device."""
    if flat.numel():
        lo, hi = (int(x) for x in torch.stack([flat.min(), flat.max()]).cpu())
        if lo < 0 or hi >= n:
            raise ValueError(text % (lo, hi, n))


def check_float32(name, t, first=None, first_name=None):
    """Refuses a tensor that is not float32 or, given the call's first operand, not on its device."""
    if t.dtype != torch.float32:
        raise ValueError('%s must be float32, got %s' % (name, t.dtype))
    if first is not None and t.device != first.device:
        raise ValueError('%s is on %s, the %s on %s' % (name, t.device, first_name, first.device))


def check_operand(name, t, shape, first=None, first_name=None):
    """Refuses an operand that is no tensor of `shape` or of [B] + `shape`, then what `check_float32` refuses (written out:
    this runs in every call, and a nested call costs what the checks do)."""
    rank = len(shape)
    if not isinstance(t, torch.Tensor) or t.dim() not in (rank, rank + 1) or tuple(t.shape[-rank:]) != shape:
        dims = ', '.join(str(s) for s in shape)
        raise ValueError('%s must have shape [%s] or [B, %s], got %s' % (name, dims, dims, tuple(getattr(t, 'shape', ())),))
    if t.dtype != torch.float32:
        raise ValueError('%s must be float32, got %s' % (name, t.dtype))
    if first is not None and t.device != first.device:
        raise ValueError('%s is on %s, the %s on %s' % (name, t.device, first_name, first.device))


def check_index_device(stage, kind, argument, index, first_name, first):
    """Refuses an index object (a `kind`, passed as `argument`) that is not on the device of the call's first operand."""
    if index.device != first.device:
        raise ValueError('%s: the %s is on %s, the %s on %s (use %s.to(device))' % (stage, kind, index.device, first_name, first.device, argument))


def scene_count(stage, *operands):
    """The scene count of a call, from (name, tensor, rank of its batched form) per operand: -> (B, batched).

    An operand shared by the scenes has no leading B and goes to the C ABI with a scene count of 1; one with a leading B has
    one value per scene.  The per-scene operands must agree on B (at most 65535); the outputs are batched if any operand is."""
    scenes = [(int(t.shape[0]), name) for name, t, rank in operands if t.dim() == rank]
    for b, name in scenes[1:]:
        if b != scenes[0][0]:
            raise ValueError('%s: %d scenes of %s, %d of %s' % (stage, scenes[0][0], scenes[0][1], b, name))
    B = scenes[0][0] if scenes else 1
    if B > 65535:
        raise ValueError('%s: %d scenes, at most 65535' % (stage, B))
    return B, bool(scenes)


def require_gpu(t, function):
    if not t.is_cuda:
        raise RuntimeError('%s runs on an MI355X only; there is no CPU fallback' % function)


def ptr(t):
    """The address of a tensor as the C ABI takes it: NULL for a missing or an empty one."""
    return t.data_ptr() or None if t is not None else None


def rows_in_place(t, width):
    """(tensor to pass, element stride between rows) such that row i of `width` floats starts at data_ptr + 4 * i * stride: a
    slice `gbuffer[..., a:a + width]` of a contiguous G-buffer (or the first or last channels of an RGBA image) is read in
    place, anything else is made contiguous.  The (u, v) pairs of the texture look-ups and the colours of `shade_gbuffer`."""
    if t.stride(-1) == 1 and t.dim() >= 2:
        step = t.stride(-2)
        ok = step >= width
        expect = step
        for d in range(t.dim() - 2, -1, -1):
            if t.stride(d) != expect:
                ok = False
                break
            expect *= t.shape[d]
        if ok:
            return t, step
    return t.contiguous(), width


def call(function, dev, *arguments, check=_lib.check):
    """One call into the C ABI: on `dev`, with its current stream as the last argument; a failure raises (`check`; texture has its own)."""
    with _ops._on_device(dev):
        rc = function(*arguments, _ops._stream_handle(dev))
    check(rc)


def grad_outputs(operands, want, empty_call):
    """The gradient outputs of a backward, like the operands (contiguous float32; one that was not given is None and wants
    none); None where not wanted, zeroed for an empty call, which launches nothing.  Fresh on every call: the node may be
    differentiated again (retain_graph=True)."""
    grads = [torch.empty_like(t) if on else None for t, on in zip(operands, want)]
    return [g.zero_() if g is not None else None for g in grads] if empty_call else grads


def dense_grads(grad_out, widths, want, empty_call):
    """The gradient outputs of tensors that stand beside a G-buffer (colours, material, a normal map: `widths` their channels):
    dense float32 [..., width] over the pixels of `grad_out`, whatever the tensors' own strides; None where not wanted,
    zeroed for an empty call, as `grad_outputs`."""
    grads = [grad_out.new_empty(tuple(grad_out.shape[:-1]) + (w,), dtype=torch.float32) if on else None for w, on in zip(widths, want)]
    return [g.zero_() if g is not None else None for g in grads] if empty_call else grads


def float32_contiguous(*grads):
    """The incoming gradients of a backward with several outputs, as the kernels read them; None (an output nobody used) stays
    None."""
    return [g.to(torch.float32).contiguous() if g is not None else None for g in grads]


def scratch(dev, nbytes):
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
