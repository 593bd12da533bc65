"""Texture look-up for deferred shaders: the helpers of the reference's samples/textured.py:16-61.

`sample_texture_uv` is the fused path -- one HIP kernel for `sample_texture(texture, uvs_to_pixel_indices(uvs, shape,
mode), filter)` and one for its gradient (include/dirt_hip.h: dirt_texture_sample_forward / _backward), reading the
(u, v) pairs in place from a G-buffer slice.  `uvs_to_pixel_indices` and `sample_texture` are the reference's two
functions over torch tensors (same names and arguments), kept for scripts that call them separately; both routes give
the same values bit for bit.

`filter='trilinear'` samples a mip pyramid (`mip_pyramid`) at a level of detail given per look-up or taken from the
screen-space footprint of the (u, v) image (dirt_texture_mip.hip; specification in DESIGN.md §7).

`sample_texture_uv_batch` and `mip_pyramid_batch` are the same two for a texture per scene, [B, Ht, Wt, C]: every pass is one
launch for all scenes (the dirt_texture_*_batch entry points), not a Python loop of B calls."""
import ctypes
import functools
import math

import torch

from . import _lib
from . import _stage


def uvs_to_pixel_indices(uvs, texture_shape, mode='repeat'):
    """[*, 2] (u, v) with (0, 0) at the TOP-LEFT of the image -> [*, 2] fractional (row, column) indices
    (samples/textured.py:16-26).  `texture_shape` = (height, width)."""
    uvs = uvs.flip(-1)  # x, y coordinates -> y, x indices
    shape = torch.as_tensor(texture_shape, dtype=uvs.dtype, device=uvs.device)
    if mode == 'repeat':
        return torch.remainder(uvs, 1.) * shape
    elif mode == 'clamp':
        return torch.clamp(uvs, 0., 1.) * shape
    raise NotImplementedError(mode)


def sample_texture(texture, indices, mode='bilinear'):
    """texture [Ht, Wt, C], fractional (row, column) `indices` [*, 2] -> [*, C] (samples/textured.py:29-60).

    Bilinear weights are the reference's (fraction of the index, no half-texel shift).  Where the reference's
    `gather_nd` would read row Ht or column Wt (an index in the last texel), the last texel is used instead."""
    ht, wt = texture.shape[0], texture.shape[1]

    def fetch(rows, cols):
        return texture[rows.clamp(0, ht - 1), cols.clamp(0, wt - 1)]

    if mode == 'nearest':
        idx = indices.to(torch.int64)  # truncation, as tf.cast
        return fetch(idx[..., 0], idx[..., 1])
    elif mode == 'bilinear':
        floor = torch.floor(indices)
        frac = indices - floor
        r, c = floor[..., 0].to(torch.int64), floor[..., 1].to(torch.int64)
        fr, fc = frac[..., :1], frac[..., 1:]
        return (fetch(r, c) * (1. - fc) * (1. - fr) + fetch(r, c + 1) * fc * (1. - fr)
                + fetch(r + 1, c) * (1. - fc) * fr + fetch(r + 1, c + 1) * fc * fr)
    raise NotImplementedError(mode)


def _check(rc):
    """A return code of a texture entry point -> ValueError with dirt_texture_last_error()'s text.  Every non-zero code, DIRT_E_HIP
    included: _lib.check raises RuntimeError for that one, and following it here would change what callers catch."""
    if rc:
        raise ValueError(_lib.load().dirt_texture_last_error().decode())


_call = functools.partial(_stage.call, check=_check)   # (entry point, device, its arguments but the stream): raises as `_check` says


def _check_texture(texture, who, batch=False):
    """One texture [height, width, channels], or with `batch` a texture per scene."""
    name, dims, axes = ('textures', 4, 'scenes, height, width, channels') if batch else ('texture', 3, 'height, width, channels')
    if texture.dim() != dims:
        raise ValueError('%s expects %s to be %dD [%s], got shape %s' % (who, name, dims, axes, tuple(texture.shape)))


def _lookup_flags(mode, filter, lod, lod_bias, mask, max_level):
    """`mode` and `filter` as the entry points' flags; the four keyword arguments of a trilinear look-up are refused with any other filter."""
    if filter != 'trilinear' and (lod is not None or lod_bias != 0.0 or mask is not None or max_level is not None):
        raise ValueError("lod, lod_bias, mask and max_level apply to filter='trilinear' only (got filter=%r)" % (filter,))
    return {'repeat': 0, 'clamp': _lib.TEX_CLAMP}[mode] | {'bilinear': 0, 'trilinear': 0, 'nearest': _lib.TEX_NEAREST}[filter]


def _check_lookup(texture, uvs):
    _check_texture(texture, 'sample_texture_uv')
    if uvs.dim() < 1 or uvs.shape[-1] != 2:
        raise ValueError('sample_texture_uv expects uvs of shape [..., 2], got %s' % (tuple(uvs.shape),))
    if texture.device != uvs.device:
        raise ValueError('texture and uvs must be on the same device (%s vs %s)' % (texture.device, uvs.device))


def _check_max_level(max_level):
    if max_level is not None and (isinstance(max_level, bool) or not isinstance(max_level, int) or max_level < 0):
        raise ValueError('max_level must be a non-negative int or None, got %r' % (max_level,))


def _pixel_grid(uv_shape, footprint=False):
    """The look-ups of a (u, v) shape as an image -> (rows, cols, image_rows): the last pixel axis is a row, everything before it stacks
    rows ([H, W, 2]; [B, H, W, 2]); a flat [n, 2] list is one row.  `image_rows`: of each stacked image, for a `footprint` level of detail."""
    n = math.prod(int(d) for d in uv_shape[:-1])
    cols = int(uv_shape[-2]) if len(uv_shape) >= 3 else n
    rows = n // cols if cols else 0
    return rows, cols, int(uv_shape[-3]) if footprint and rows else 1


def _pairs_in_place(uvs):
    """(tensor to pass, element stride between pairs) such that pair i starts at data_ptr + 4 * i * stride: a slice
    `gbuffer[..., a:a+2]` of a contiguous G-buffer is read in place, anything else is made contiguous."""
    return _stage.rows_in_place(uvs, 2)


_BATCHED = {'sample_forward': 'sample_batch_forward', 'sample_backward_image': 'sample_batch_backward_image', 'mip_build': 'mip_build_batch',
            'mip_collapse': 'mip_collapse_batch', 'sample_mip_forward': 'sample_mip_batch_forward', 'sample_mip_backward': 'sample_mip_batch_backward'}


def _call_entry(name, scenes, dev, pointers, *sizes):
    """dirt_texture_<name>(*pointers, *sizes) for one texture (`scenes` None), else its batched form, which takes the scene count after
    the pointers and the sizes per scene; no scenes, no call."""
    if scenes is None:
        _call(getattr(_lib.load(), 'dirt_texture_' + name), dev, *pointers, *sizes)
    elif scenes:
        _call(getattr(_lib.load(), 'dirt_texture_' + _BATCHED[name]), dev, *pointers, scenes, *sizes)


def _scene_grid(uv_shape, scenes, footprint=False):
    """`_pixel_grid` of one texture's look-ups: all of them, or those of one scene of a batch (everything after the leading axis)."""
    return _pixel_grid(uv_shape if scenes is None else uv_shape[1:], footprint)


class _SampleTextureUV(torch.autograd.Function):
    """texture [Ht, Wt, C] and `scenes` None, or textures [scenes, Ht, Wt, C] with uvs [scenes, ..., 2]."""

    @staticmethod
    def forward(ctx, texture, uvs, flags, scenes):
        texture = texture.contiguous()
        src, stride = _pairs_in_place(uvs)
        rows, cols, _ = _scene_grid(uvs.shape, scenes)
        ht, wt, ct = (int(d) for d in texture.shape[-3:])
        out = torch.empty(tuple(uvs.shape[:-1]) + (ct,), dtype=torch.float32, device=texture.device)
        _call_entry('sample_forward', scenes, texture.device, (texture.data_ptr(), src.data_ptr(), out.data_ptr()), rows * cols, ht, wt, ct, stride, flags)
        ctx.save_for_backward(texture, src)
        ctx.meta = (stride, flags, tuple(uvs.shape), scenes)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        texture, src = ctx.saved_tensors
        stride, flags, uv_shape, scenes = ctx.meta
        ht, wt, ct = (int(d) for d in texture.shape[-3:])
        grad_out = grad_out.contiguous().to(torch.float32)
        grad_texture = torch.empty_like(texture)
        grad_uvs = torch.empty(uv_shape, dtype=torch.float32, device=texture.device) if ctx.needs_input_grad[1] else None
        rows, cols, _ = _scene_grid(uv_shape, scenes)
        _call_entry('sample_backward_image', scenes, texture.device, (texture.data_ptr(), src.data_ptr(), grad_out.data_ptr(),
                    grad_texture.data_ptr(), _stage.ptr(grad_uvs)), rows, cols, ht, wt, ct, stride, 2, flags)
        return grad_texture, grad_uvs, None, None


def sample_texture_uv(texture, uvs, mode='repeat', filter='bilinear', *, lod=None, lod_bias=0.0, mask=None, max_level=None):
    """Fused `sample_texture(texture, uvs_to_pixel_indices(uvs, texture.shape[:2], mode), filter)`
    (samples/textured.py:16-61, as its shader_fn uses them, :116-141): texture [Ht, Wt, C] float32, uvs [*, 2] with
    (0, 0) at the top-left of the image -> [*, C].  Differentiable with respect to the texture and the coordinates.

    filter='trilinear' blends bilinear samples of two adjacent levels of the texture's mip pyramid.  The
    level of detail is `lod` + `lod_bias` when `lod` (shaped like uvs[..., 0]) is given, else log2 of the screen-space
    footprint of (u, v) + `lod_bias`, which needs `uvs` as images [..., H, W, 2]; `mask` [..., H, W] (e.g. gbuffer[..., 0],
    read in place) marks the pixels whose (u, v) count as neighbours.  `max_level` caps the pyramid.  Also differentiable
    with respect to `lod`; the footprint's level is held constant.  The four keyword arguments apply to 'trilinear' only."""
    flags = _lookup_flags(mode, filter, lod, lod_bias, mask, max_level)
    if filter == 'trilinear':
        return _sample_trilinear(texture, uvs, flags, lod, lod_bias, mask, max_level)
    _check_lookup(texture, uvs)
    _stage.require_gpu(texture, 'dirt_amd.texture.sample_texture_uv')
    return _SampleTextureUV.apply(texture.to(torch.float32), uvs.to(torch.float32), flags, None)


# ---- mip pyramid and trilinear look-up (dirt_texture_mip.hip) ----------------------------------------------------------

def _mip_geometry(ht, wt, ct, max_level):
    """-> (level count, packed floats, [(offset, H_k, W_k)] per level) of the pyramid of an ht x wt x ct texture."""
    _check_max_level(max_level)
    lib = _lib.load()
    floats = ctypes.c_longlong(0)
    levels = lib.dirt_texture_mip_levels(ht, wt, ct, -1 if max_level is None else max_level, ctypes.byref(floats))
    _check(min(levels, 0))   # a level count (>= 1), or an error code
    geo, off = [], 0
    for k in range(levels):
        h, w = max(ht >> k, 1), max(wt >> k, 1)
        geo.append((off, h, w))
        off += h * w * ct
    assert off == floats.value
    return levels, floats.value, geo


class _MipPyramid(torch.autograd.Function):
    """texture [Ht, Wt, C] -> [floats], or textures [scenes, Ht, Wt, C] -> [scenes, floats]."""

    @staticmethod
    def forward(ctx, texture, levels, floats, scenes):
        texture = texture.contiguous()
        ht, wt, ct = (int(d) for d in texture.shape[-3:])
        pyr = torch.empty(tuple(texture.shape[:-3]) + (floats,), dtype=torch.float32, device=texture.device)
        _call_entry('mip_build', scenes, texture.device, (texture.data_ptr(), pyr.data_ptr()), ht, wt, ct, levels)
        ctx.meta = (ht, wt, ct, levels, scenes)
        return pyr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_pyr):
        ht, wt, ct, levels, scenes = ctx.meta
        grad_pyr = grad_pyr.contiguous().to(torch.float32)
        grad_texture = torch.empty(tuple(grad_pyr.shape[:-1]) + (ht, wt, ct), dtype=torch.float32, device=grad_pyr.device)
        _call_entry('mip_collapse', scenes, grad_pyr.device, (grad_pyr.data_ptr(), grad_texture.data_ptr()), ht, wt, ct, levels)
        return grad_texture, None, None, None


def mip_pyramid(texture, max_level=None):
    """texture [Ht, Wt, C] -> [level 0, level 1, ...]: each level [max(Ht >> k, 1), max(Wt >> k, 1), C] the 2 x 2 (or 2 x 1)
    means of the one below, while every dimension is even or 1 and up to `max_level`.  The levels are views
    into one packed buffer (level 0 a copy of the texture); differentiable with respect to the texture."""
    _check_texture(texture, 'mip_pyramid')
    _stage.require_gpu(texture, 'dirt_amd.texture.mip_pyramid')
    ht, wt, ct = (int(d) for d in texture.shape)
    levels, floats, geo = _mip_geometry(ht, wt, ct, max_level)
    packed = _MipPyramid.apply(texture.to(torch.float32), levels, floats, None)
    return [packed[o:o + h * w * ct].view(h, w, ct) for (o, h, w) in geo]


def _scalars_in_place(x):
    """(tensor to pass, element stride between consecutive values) for a float32 tensor whose elements lie a constant stride
    apart in row-major order (a slice `gbuffer[..., 0]` of a contiguous G-buffer); anything else is made contiguous float32."""
    if x.dtype == torch.float32 and x.dim() >= 1:
        step = x.stride(-1)
        ok = step >= 1
        expect = step
        for d in range(x.dim() - 1, -1, -1):
            if x.shape[d] != 1 and x.stride(d) != expect:
                ok = False
                break
            expect *= x.shape[d]
        if ok:
            return x, step
    return x.to(torch.float32).contiguous(), 1


class _SampleTextureMip(torch.autograd.Function):
    """texture [Ht, Wt, C] and `scenes` None, or textures [scenes, Ht, Wt, C] with uvs [scenes, ..., 2] (pyramids and scratch [scenes, floats])."""

    @staticmethod
    def forward(ctx, texture, uvs, lod, mask, flags, lod_bias, max_level, scenes):
        texture = texture.contiguous()
        ht, wt, ct = (int(d) for d in texture.shape[-3:])
        levels, floats, _ = _mip_geometry(ht, wt, ct, max_level)
        src, stride = _pairs_in_place(uvs)
        rows, cols, image_rows = _scene_grid(uvs.shape, scenes, footprint=lod is None)
        lod_t = lod.to(torch.float32).contiguous() if lod is not None else None
        mask_t, mask_stride = _scalars_in_place(mask) if mask is not None else (None, 1)
        pyr = torch.empty(tuple(texture.shape[:-3]) + (floats,), dtype=torch.float32, device=texture.device)
        out = torch.empty(tuple(uvs.shape[:-1]) + (ct,), dtype=torch.float32, device=texture.device)
        _call_entry('mip_build', scenes, texture.device, (texture.data_ptr(), pyr.data_ptr()), ht, wt, ct, levels)
        _call_entry('sample_mip_forward', scenes, texture.device, (pyr.data_ptr(), src.data_ptr(), _stage.ptr(lod_t), _stage.ptr(mask_t), out.data_ptr()),
                    rows, cols, image_rows, ht, wt, ct, levels, stride, mask_stride, float(lod_bias), flags)
        ctx.save_for_backward(pyr, src, lod_t, mask_t)
        ctx.meta = (stride, mask_stride, flags, float(lod_bias), tuple(uvs.shape), rows, cols, image_rows, ht, wt, ct, levels, scenes)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pyr, src, lod_t, mask_t = ctx.saved_tensors
        stride, mask_stride, flags, lod_bias, uv_shape, rows, cols, image_rows, ht, wt, ct, levels, scenes = ctx.meta
        dev = pyr.device
        grad_out = grad_out.contiguous().to(torch.float32)
        scratch = torch.empty_like(pyr)    # the pyramid-shaped gradient, cleared by the call
        grad_texture = torch.empty(tuple(pyr.shape[:-1]) + (ht, wt, ct), dtype=torch.float32, device=dev)
        grad_uvs = torch.empty(uv_shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        grad_lod = torch.empty(uv_shape[:-1], dtype=torch.float32, device=dev) if lod_t is not None and ctx.needs_input_grad[2] else None
        _call_entry('sample_mip_backward', scenes, dev, (pyr.data_ptr(), src.data_ptr(), _stage.ptr(lod_t), _stage.ptr(mask_t), grad_out.data_ptr(),
                    scratch.data_ptr(), grad_texture.data_ptr(), _stage.ptr(grad_uvs), _stage.ptr(grad_lod)), rows, cols, image_rows,
                    ht, wt, ct, levels, stride, 2, mask_stride, lod_bias, flags)
        return grad_texture, grad_uvs, grad_lod, None, None, None, None, None


def _check_trilinear(uvs, lod, mask, max_level, image_dims=3):
    """The keyword arguments of a trilinear look-up; `image_dims`: the axes uvs needs for a footprint level of detail."""
    _check_max_level(max_level)
    for name, x in (('lod', lod), ('mask', mask)):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != tuple(uvs.shape[:-1]):
            raise ValueError('%s must be a tensor shaped like uvs[..., 0] %s, got %s' % (name, tuple(uvs.shape[:-1]), tuple(getattr(x, 'shape', ()))))
        if x.device != uvs.device:
            raise ValueError('%s and uvs must be on the same device (%s vs %s)' % (name, x.device, uvs.device))
    if lod is None and uvs.dim() < image_dims:
        raise ValueError("filter='trilinear' without lod takes the level of detail from neighbouring pixels: uvs must be images "
                         "[..., H, W, 2], got %s" % (tuple(uvs.shape),))
    if lod is not None and mask is not None:
        raise ValueError('mask marks the neighbours of the footprint level of detail; it does not apply with an explicit lod')


def _sample_trilinear(texture, uvs, flags, lod, lod_bias, mask, max_level):
    _check_lookup(texture, uvs)
    _check_trilinear(uvs, lod, mask, max_level)
    _stage.require_gpu(texture, 'dirt_amd.texture.sample_texture_uv')
    return _SampleTextureMip.apply(texture.to(torch.float32), uvs.to(torch.float32), lod, mask, flags, float(lod_bias), max_level, None)


# ---- a texture per scene: the same kernels, the scene a launch dimension -------------------------------------

def _require_gpu_batch(t, name, who):
    if not t.is_cuda:
        raise ValueError('%s runs on an MI355X only and has no CPU fallback: %s is on %s' % (who, name, t.device))


def sample_texture_uv_batch(textures, uvs, mode='repeat', filter='bilinear', *, lod=None, lod_bias=0.0, mask=None, max_level=None):
    """`sample_texture_uv` with a texture per scene, every pass one launch for all scenes: textures [B, Ht, Wt, C] float32,
    uvs [B, ..., 2] -> [B, ..., C], equal to torch.stack([sample_texture_uv(textures[b], uvs[b], mode, filter, ...) for b in
    range(B)]) with `lod` and `mask` (shaped like uvs[..., 0]) indexed alike.  Everything after the leading axis of uvs is
    scene b's and reads textures[b]; the footprint level of detail of 'trilinear' never looks across images or scenes, and
    without `lod` needs uvs as images [B, ..., H, W, 2].  A slice gbuffer[..., a:a+2] of a contiguous [B, H, W, Cg] G-buffer
    and mask=gbuffer[..., 0] are read in place.  Differentiable with respect to textures, uvs and lod."""
    who = 'sample_texture_uv_batch'
    flags = _lookup_flags(mode, filter, lod, lod_bias, mask, max_level)
    _check_texture(textures, who, batch=True)
    if uvs.dim() < 2 or uvs.shape[-1] != 2:
        raise ValueError('%s expects uvs of shape [scenes, ..., 2], got %s' % (who, tuple(uvs.shape)))
    if uvs.shape[0] != textures.shape[0]:
        raise ValueError('%s: %d scenes of textures, %d of uvs' % (who, textures.shape[0], uvs.shape[0]))
    if filter == 'trilinear':
        _check_trilinear(uvs, lod, mask, max_level, image_dims=4)
    if textures.device != uvs.device:
        raise ValueError('textures and uvs must be on the same device (%s vs %s)' % (textures.device, uvs.device))
    _require_gpu_batch(textures, 'textures', who)
    scenes = int(textures.shape[0])
    if filter == 'trilinear':
        return _SampleTextureMip.apply(textures.to(torch.float32), uvs.to(torch.float32), lod, mask, flags, float(lod_bias), max_level, scenes)
    return _SampleTextureUV.apply(textures.to(torch.float32), uvs.to(torch.float32), flags, scenes)


def mip_pyramid_batch(textures, max_level=None):
    """`mip_pyramid` of B textures [B, Ht, Wt, C] in one launch per level group -> [level 0, level 1, ...], level k
    [B, max(Ht >> k, 1), max(Wt >> k, 1), C].  The levels are views into one packed buffer [B, pyramid floats]: scene b's
    pyramid after scene b - 1's, each laid out as `mip_pyramid`'s.  Differentiable with respect to the textures."""
    _check_texture(textures, 'mip_pyramid_batch', batch=True)
    _require_gpu_batch(textures, 'textures', 'mip_pyramid_batch')
    scenes, ht, wt, ct = (int(d) for d in textures.shape)
    levels, floats, geo = _mip_geometry(ht, wt, ct, max_level)
    packed = _MipPyramid.apply(textures.to(torch.float32), levels, floats, scenes)
    return [packed[:, o:o + h * w * ct].view(scenes, h, w, ct) for (o, h, w) in geo]
