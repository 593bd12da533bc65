"""Texture look-up for deferred shaders: the helpers of the reference's samples/textured.py:16-61.

`sample_texture_uv` is the fused path -- one HIP kernel for `sample_texture(texture, uvs_to_pixel_indices(uvs, shape,
mode), filter)` and one for its gradient (include/dirt_hip.h: dirt_texture_sample_forward / _backward), reading the
(u, v) pairs in place from a G-buffer slice.  `uvs_to_pixel_indices` and `sample_texture` are the reference's two
functions over torch tensors (same names and arguments), kept for scripts that call them separately; both routes give
the same values bit for bit.

`filter='trilinear'` samples a mip pyramid (`mip_pyramid`) at a level of detail given per look-up or taken from the
screen-space footprint of the (u, v) image (dirt_texture_mip.hip; specification in DESIGN.md §7).

`sample_texture_uv_batch` and `mip_pyramid_batch` are the same two for a texture per scene, [B, Ht, Wt, C]: every pass is one
launch for all scenes (the dirt_texture_*_batch entry points), not a Python loop of B calls.

`sample_texture_cube` looks a cube map [6, N, N, C] up by direction (an environment map; dirt_texture_cube.hip), with the
same three filters; `directions_to_cube_indices` and `sample_cube` are its pure-torch form, as `uvs_to_pixel_indices` and
`sample_texture` are the flat look-up's.

`prefilter_cube` makes the GGX-prefiltered pyramid of an environment cube (a `CubePyramid`: level k the cube's box-filtered
level k convolved with a GGX lobe of roughness r_k; dirt_envmap.hip), `convolve_cube` one such convolution (or the cosine
one, the irradiance), and `sample_cube_pyramid` is the trilinear cube look-up in a pyramid the caller made -- `cube_pyramid`
the box-filtered one.  `cube_texel_directions` and `convolve_cube_dense` are the convolution's pure-torch form for small cubes.

`panorama_to_cube` resamples a lat-long (equirectangular) panorama [H, W, C] into such a cube and `cube_to_panorama` a cube
into a panorama, supersampled and under an optional rotation, with gradients to the sampled operand and to the rotation
(dirt_panorama.hip); `panorama_to_cube_dense` and `cube_to_panorama_dense`, over `panorama_texel_directions`,
`directions_to_panorama_indices` and `sample_panorama`, are their pure-torch form and their specification."""
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


# ---- cube map: a texture indexed by a direction (dirt_texture_cube.hip; specification in DESIGN.md §7) ---------------------------

def directions_to_cube_indices(directions, size):
    """[..., 3] directions (not normalised) -> (face int64 [...], fractional (row, column) indices float32 [..., 2] into a
    `size` x `size` face, valid bool [...]): the major axis picks the face (+X, -X, +Y, -Y, +Z, -Z = 0..5, ties to X before Y
    before Z), the other two components over its magnitude give the GL texel-centre index, clamped to the face.  A direction
    that is not finite or is all zero is not valid: face 0, index 0, and no gradient.  Pure torch, on any device, differentiable;
    `sample_cube(cube, *directions_to_cube_indices(directions, size))` is what `sample_texture_cube` fuses."""
    with torch.no_grad():
        valid = torch.isfinite(directions).all(-1) & (directions.abs().amax(-1) > 0)
    d = torch.where(valid.unsqueeze(-1), directions, torch.zeros_like(directions))
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    a = torch.where(is_x, ax, torch.where(is_y, ay, az))
    pos = torch.where(is_x, x, torch.where(is_y, y, z)) > 0
    face = torch.where(is_x, 0, torch.where(is_y, 2, 4)) + (~pos).to(torch.int64)
    sc = torch.where(is_x, torch.where(pos, -z, z), torch.where(is_y, x, torch.where(pos, x, -x)))
    tc = torch.where(is_y, torch.where(pos, z, -z), -y)
    a = torch.where(valid, a, torch.ones_like(a))
    indices = torch.stack([tc, sc], -1) / a.unsqueeze(-1)
    indices = (((indices + 1.) * 0.5) * float(size) - 0.5).clamp(0., float(size - 1))
    zero = torch.zeros_like(face)
    return torch.where(valid, face, zero), torch.where(valid.unsqueeze(-1), indices, torch.zeros_like(indices)), valid


def sample_cube(cube, face, indices, valid, mode='bilinear'):
    """cube [6, N, N, C], and per look-up the face, the fractional (row, column) `indices` [..., 2] and `valid` of
    `directions_to_cube_indices` -> [..., C]: the bilinear blend of the face's four texels around the index (taps never leave
    the face), or with 'nearest' the texel whose centre is closest; 0 where not valid.  Pure torch, differentiable."""
    n = cube.shape[1]

    def fetch(rows, cols):
        return cube[face, rows.clamp(0, n - 1), cols.clamp(0, n - 1)]

    if mode == 'nearest':
        idx = (indices + 0.5).to(torch.int64)
        out = fetch(idx[..., 0], idx[..., 1])
    elif mode == 'bilinear':
        floor = torch.floor(indices)
        frac = indices - floor
        r, c = floor[..., 0].to(torch.int64), floor[..., 1].to(torch.int64)
        fr, fc = frac[..., :1], frac[..., 1:]
        out = (fetch(r, c) * (1. - fc) * (1. - fr) + fetch(r, c + 1) * fc * (1. - fr)
               + fetch(r + 1, c) * (1. - fc) * fr + fetch(r + 1, c + 1) * fc * fr)
    else:
        raise NotImplementedError(mode)
    return torch.where(valid.unsqueeze(-1), out, torch.zeros_like(out))


class _SampleTextureCube(torch.autograd.Function):
    """cube [6, N, N, C], directions [..., 3]; `lod` given: trilinear over a pyramid per face (pyramid and scratch [6, floats])."""

    @staticmethod
    def forward(ctx, cube, directions, lod, flags, lod_bias, max_level):
        cube = cube.contiguous()
        n, ct = int(cube.shape[1]), int(cube.shape[3])
        lib = _lib.load()
        src, stride = _stage.rows_in_place(directions, 3)
        rows, cols, _ = _pixel_grid(directions.shape)
        lod_t = lod.to(torch.float32).contiguous() if lod is not None else None
        levels, pyr = 1, cube      # (one level: the packed pyramids are the cube itself)
        if lod is not None:
            levels, floats, _ = _mip_geometry(n, n, ct, max_level)
            pyr = torch.empty((6, floats), dtype=torch.float32, device=cube.device)
            _call_entry('mip_build', 6, cube.device, (cube.data_ptr(), pyr.data_ptr()), n, n, ct, levels)
        out = torch.empty(tuple(directions.shape[:-1]) + (ct,), dtype=torch.float32, device=cube.device)
        _call(lib.dirt_texture_cube_forward, cube.device, pyr.data_ptr(), _stage.ptr(src), _stage.ptr(lod_t), _stage.ptr(out), rows * cols, n, ct, levels,
              stride, float(lod_bias), flags)
        ctx.save_for_backward(pyr, src, lod_t)
        ctx.meta = (stride, flags, float(lod_bias), tuple(directions.shape), rows, cols, n, ct, levels)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pyr, src, lod_t = ctx.saved_tensors
        stride, flags, lod_bias, dir_shape, rows, cols, n, ct, levels = ctx.meta
        dev = pyr.device
        grad_out = grad_out.contiguous().to(torch.float32)
        scratch = torch.empty((6, pyr.numel() // 6), dtype=torch.float32, device=dev)   # every level's gradient, cleared by the call
        grad_dirs = torch.empty(dir_shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        grad_lod = torch.empty(dir_shape[:-1], dtype=torch.float32, device=dev) if lod_t is not None and ctx.needs_input_grad[2] else None
        _call(_lib.load().dirt_texture_cube_backward, dev, pyr.data_ptr(), _stage.ptr(src), _stage.ptr(lod_t), _stage.ptr(grad_out), scratch.data_ptr(),
              _stage.ptr(grad_dirs), _stage.ptr(grad_lod), rows, cols, n, ct, levels, stride, 3, lod_bias, flags)
        grad_cube = None
        if ctx.needs_input_grad[0] and levels == 1:
            grad_cube = scratch.view(6, n, n, ct)
        elif ctx.needs_input_grad[0]:
            grad_cube = torch.empty((6, n, n, ct), dtype=torch.float32, device=dev)
            _call_entry('mip_collapse', 6, dev, (scratch.data_ptr(), grad_cube.data_ptr()), n, n, ct, levels)
        return grad_cube, grad_dirs, grad_lod, None, None, None


def sample_texture_cube(cube, directions, filter='bilinear', *, lod=None, lod_bias=0.0, max_level=None):
    """Fused `sample_cube(cube, *directions_to_cube_indices(directions, N), filter)`: cube [6, N, N, C] float32 with its
    faces in OpenGL order (+X, -X, +Y, -Y, +Z, -Z), directions [..., 3] (not normalised; a slice gbuffer[..., a:a+3] of a
    contiguous G-buffer is read in place) -> [..., C].  A direction that is not finite or is all zero -- a background pixel's
    normal -- gives 0 and takes no part in any gradient, so no mask is needed.  Each face clamps to its own edges (no
    seamless filtering).  Differentiable with respect to the cube and the directions.

    filter='trilinear' blends two adjacent levels of a mip pyramid per face (`mip_pyramid_batch(cube)`, capped by
    `max_level`) at the level of detail `lod` + `lod_bias`; `lod`, shaped like directions[..., 0], is required (e.g. a
    roughness times the top level) and is differentiable too.  The three keyword arguments apply to 'trilinear' only."""
    who = 'sample_texture_cube'
    if filter not in ('bilinear', 'nearest', 'trilinear'):
        raise ValueError("%s: filter must be 'bilinear', 'nearest' or 'trilinear', got %r" % (who, filter))
    if filter != 'trilinear' and (lod is not None or lod_bias != 0.0 or max_level is not None):
        raise ValueError("lod, lod_bias and max_level apply to filter='trilinear' only (got filter=%r)" % (filter,))
    if not isinstance(cube, torch.Tensor) or cube.dim() != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or 0 in cube.shape:
        raise ValueError('%s expects cube to be 4D [6, size, size, channels], got shape %s' % (who, tuple(getattr(cube, 'shape', ()))))
    if not isinstance(directions, torch.Tensor) or directions.dim() < 1 or directions.shape[-1] != 3:
        raise ValueError('%s expects directions of shape [..., 3], got %s' % (who, tuple(getattr(directions, 'shape', ()))))
    for name, t in (('cube', cube), ('directions', directions)):
        if not t.is_floating_point():
            raise ValueError('%s: %s must be a floating-point tensor, got %s' % (who, name, t.dtype))
    if cube.device != directions.device:
        raise ValueError('cube and directions must be on the same device (%s vs %s)' % (cube.device, directions.device))
    if filter == 'trilinear':
        _check_max_level(max_level)
        if lod is None:
            raise ValueError("%s: filter='trilinear' needs lod (a level of detail from the footprint of the directions is not supported)" % who)
        if not isinstance(lod, torch.Tensor) or tuple(lod.shape) != tuple(directions.shape[:-1]):
            raise ValueError('lod must be a tensor shaped like directions[..., 0] %s, got %s' % (tuple(directions.shape[:-1]), tuple(getattr(lod, 'shape', ()))))
        if lod.device != directions.device:
            raise ValueError('lod and directions must be on the same device (%s vs %s)' % (lod.device, directions.device))
    _stage.require_gpu(cube, 'dirt_amd.texture.sample_texture_cube')
    return _SampleTextureCube.apply(cube.to(torch.float32), directions.to(torch.float32), lod, _lib.TEX_NEAREST if filter == 'nearest' else 0,
                                    float(lod_bias), max_level)


# ---- prefiltered environment maps: a pyramid whose levels are the cube convolved with a lobe (dirt_envmap.hip) ---------

ROUGHNESS_MIN = 1.0 / 32.0   # the narrowest GGX lobe the filter takes; 0 is the identity


class CubePyramid:
    """A pyramid per face of a cube map in one packed buffer: `packed` [6, floats] float32 (it carries the autograd graph), laid out
    as `mip_pyramid_batch(cube)`'s, `size` and `channels` of level 0, the `levels` count, and `roughness`: the roughness each level was
    convolved at (a tuple), or None where the levels are box-filtered means.  `cube_pyramid` and `prefilter_cube` make one;
    `sample_cube_pyramid` looks it up."""

    def __init__(self, packed, size, channels, levels, roughness=None):
        self.packed, self.size, self.channels, self.levels = packed, int(size), int(channels), int(levels)
        self.roughness = None if roughness is None else tuple(float(r) for r in roughness)

    def level(self, k):
        """Level k as a view [6, n_k, n_k, C] into `packed`."""
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.levels:
            raise ValueError('CubePyramid.level: level %r of %d' % (k, self.levels))
        o, n = _cube_level(self.size, self.channels, k)
        return self.packed[:, o:o + n * n * self.channels].view(6, n, n, self.channels)


def _cube_level(size, channels, k):
    """-> (offset in floats inside a face's packed pyramid, size) of level k."""
    n = size >> k
    return (size * size - n * n) // 3 * 4 * channels, n


def _check_cube(cube, who):
    if not isinstance(cube, torch.Tensor) or cube.dim() != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or 0 in cube.shape:
        raise ValueError('%s expects cube to be 4D [6, size, size, channels], got shape %s' % (who, tuple(getattr(cube, 'shape', ()))))
    if not cube.is_floating_point():
        raise ValueError('%s: cube must be a floating-point tensor, got %s' % (who, cube.dtype))


def _check_roughness(r, who):
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not (r == 0 or ROUGHNESS_MIN <= r <= 1):
        raise ValueError('%s: roughness must be a float that is 0 or in [1/32, 1], got %r' % (who, r))
    return float(r)


def _filter_kind(kind, roughness, who):
    """-> (the entry points' kind, roughness as a float; Lambert: 1.0, which they ignore)"""
    if kind not in ('ggx', 'lambert'):
        raise ValueError("%s: kind must be 'ggx' or 'lambert', got %r" % (who, kind))
    if kind == 'lambert':
        if roughness is not None:
            raise ValueError("%s: roughness applies to kind='ggx' only (got kind='lambert', roughness=%r)" % (who, roughness))
        return _lib.ENVMAP_LAMBERT, 1.0
    if roughness is None:
        raise ValueError("%s: kind='ggx' needs a roughness" % who)
    return _lib.ENVMAP_GGX, _check_roughness(roughness, who)


def cube_texel_directions(size, device=None, dtype=torch.float32):
    """-> (directions [6, size, size, 3], unit vectors through the texel centres of a cube map's faces in OpenGL order, and
    weights [6, size, size], the texels' solid angles up to a constant: (1 + sc^2 + tc^2)^(-3/2)).  The inverse of
    `directions_to_cube_indices`: direction [f, r, c] maps back to face f, index (r, c).  Pure torch."""
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise ValueError('cube_texel_directions: size must be a positive int, got %r' % (size,))
    x = 2. * (torch.arange(size, device=device, dtype=dtype) + 0.5) / size - 1.
    tc, sc = torch.meshgrid(x, x, indexing='ij')
    one = torch.ones_like(sc)
    v = torch.stack([torch.stack(f, -1) for f in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one))])
    inv = 1. / torch.sqrt(1. + sc * sc + tc * tc)
    return v * inv[None, :, :, None], (inv * inv * inv).expand(6, size, size).contiguous()


def convolve_cube_dense(cube, roughness=None, kind='ggx'):
    """The specification of `convolve_cube` as a dense [6 N^2, 6 N^2] matrix, for small N: pure torch, on any device, in the
    cube's dtype, differentiable.  cube [6, N, N, C] -> [6, N, N, C]: every texel the mean of all texels, weighted by their solid
    angles and by k(t) of the cosine t between the two texels' directions -- the clamped cosine t+ ('lambert'), or ('ggx',
    alpha = roughness^2) t+ max(q(t) - q_c, 0) with q(t) = 1 / (1 + t+^2 (alpha^2 - 1))^2 and q_c = q(1) / 256 while
    16 alpha^2 < 1, else 0.  roughness 0 is the identity."""
    who = 'convolve_cube_dense'
    _check_cube(cube, who)
    code, r = _filter_kind(kind, roughness, who)
    if code == _lib.ENVMAP_GGX and r == 0:
        return cube.clone()
    n, ct = int(cube.shape[1]), int(cube.shape[3])
    d, w = cube_texel_directions(n, cube.device, cube.dtype)
    d = d.reshape(-1, 3)
    with torch.no_grad():   # the weights depend on the geometry alone (in place: three matrices at a time)
        e = sum((d[:, None, i] - d[None, :, i]).square_() for i in range(3))   # |d_o - d_s|^2 = 2 - 2 t: 1 - t^2 = e (1 - e / 4) without cancellation
        k = (1. - 0.5 * e).clamp_min_(0.)                  # t+
        if code == _lib.ENVMAP_GGX:
            a2 = r ** 4
            e = torch.where(k > 0, e * (1. - 0.25 * e), 1.).add_(a2 * k * k)   # 1 - t+^2 (an antipodal pair: 1), then 1 + t+^2 (alpha^2 - 1)
            q = e.reciprocal_().mul_(a2).square_()         # q(t) alpha^4
            k.mul_(q.sub_(1. / 256. if 16. * a2 < 1. else 0.).clamp_min_(0.))
        del e
        k.mul_(w.reshape(1, -1))
        k.div_(k.sum(1, keepdim=True))
    return (k @ cube.reshape(-1, ct)).reshape(6, n, n, ct)


def _level_in_place(cube):
    """(tensor to pass, floats between its faces): a `CubePyramid.level(k)` view -- dense faces a constant stride apart -- is read in
    place, anything else is made contiguous."""
    _, n, _, ct = (int(s) for s in cube.shape)
    if cube.dtype == torch.float32 and tuple(cube.stride()[1:]) == (n * ct, ct, 1) and cube.stride(0) >= n * n * ct:
        return cube, int(cube.stride(0))
    return cube.to(torch.float32).contiguous(), n * n * ct


def _envmap_filter(src, dst, stride, norm, n, ct, alpha, code, transposed=False):
    """One level through dirt_envmap_filter_forward (`norm` written) or _backward (`norm` read); src and dst are tensors whose
    first element is the level's first of face 0, the faces of both `stride` floats apart (the entry points take one stride)."""
    lib = _lib.load()
    if transposed:
        _call(lib.dirt_envmap_filter_backward, dst.device, src.data_ptr(), norm.data_ptr(), dst.data_ptr(), n, ct, stride, alpha, code)
    else:
        _call(lib.dirt_envmap_filter_forward, dst.device, src.data_ptr(), dst.data_ptr(), norm.data_ptr(), n, ct, stride, alpha, code)


class _ConvolveCube(torch.autograd.Function):
    """cube [6, N, N, C] (faces `stride` floats apart) -> [6, N, N, C]."""

    @staticmethod
    def forward(ctx, cube, alpha, code):
        src, stride = _level_in_place(cube)
        n, ct = int(cube.shape[1]), int(cube.shape[3])
        if stride != n * n * ct:   # a level inside a packed pyramid: the output gets the same face stride (one stride per call)
            out = torch.empty((6, stride), dtype=torch.float32, device=cube.device)[:, :n * n * ct].view(6, n, n, ct)
        else:
            out = torch.empty((6, n, n, ct), dtype=torch.float32, device=cube.device)
        norm = torch.empty((6, n, n), dtype=torch.float32, device=cube.device)
        _envmap_filter(src, out, stride, norm, n, ct, alpha, code)
        ctx.save_for_backward(norm)
        ctx.meta = (n, ct, alpha, code)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        norm, = ctx.saved_tensors
        n, ct, alpha, code = ctx.meta
        grad_out = grad_out.to(torch.float32).contiguous()
        grad_cube = torch.empty_like(grad_out)
        _envmap_filter(grad_out, grad_cube, n * n * ct, norm, n, ct, alpha, code, transposed=True)
        return grad_cube, None, None


def convolve_cube(cube, roughness=None, kind='ggx'):
    """One level of an environment map convolved with a lobe on the sphere, by the HIP filter kernel: cube [6, N, N, C] float32
    (faces in OpenGL order) -> [6, N, N, C], what `convolve_cube_dense` specifies.  kind='ggx': a GGX lobe of `roughness` (a
    float, 0 -- the identity -- or in [1/32, 1]; not differentiable); kind='lambert': the clamped cosine, the cube's irradiance
    up to the factor pi (takes no roughness).  A `CubePyramid.level(k)` view is read in place.  Differentiable with respect
    to the cube: the gradient is the transposed convolution, by the same kernel.  The same bits on every run."""
    who = 'convolve_cube'
    _check_cube(cube, who)
    code, r = _filter_kind(kind, roughness, who)
    _stage.require_gpu(cube, 'dirt_amd.texture.convolve_cube')
    if code == _lib.ENVMAP_GGX and r == 0:
        return cube.to(torch.float32).clone()
    return _ConvolveCube.apply(cube if cube.dtype == torch.float32 else cube.to(torch.float32), r * r, code)


def _pyramid_geometry(cube, max_level, who):
    _check_cube(cube, who)
    _check_max_level(max_level)
    n, ct = int(cube.shape[1]), int(cube.shape[3])
    levels, floats, _ = _mip_geometry(n, n, ct, max_level)
    return n, ct, levels, floats


def cube_pyramid(cube, max_level=None):
    """The box-filtered pyramid of a cube map [6, N, N, C] as a `CubePyramid` (roughness None): `mip_pyramid_batch(cube)` with the
    six faces as scenes, the pyramid `sample_texture_cube(..., filter='trilinear')` builds for itself.  Differentiable."""
    n, ct, levels, floats = _pyramid_geometry(cube, max_level, 'cube_pyramid')
    _stage.require_gpu(cube, 'dirt_amd.texture.cube_pyramid')
    return CubePyramid(_MipPyramid.apply(cube.to(torch.float32), levels, floats, 6), n, ct, levels)


class _PrefilterCube(torch.autograd.Function):
    """cube [6, N, N, C] -> packed [6, floats]: the box pyramid, then level k convolved at roughness[k] (0: copied)."""

    @staticmethod
    def forward(ctx, cube, roughness, levels, floats):
        cube = cube.contiguous()
        n, ct = int(cube.shape[1]), int(cube.shape[3])
        dev = cube.device
        box = torch.empty((6, floats), dtype=torch.float32, device=dev)
        _call_entry('mip_build', 6, dev, (cube.data_ptr(), box.data_ptr()), n, n, ct, levels)
        packed = torch.empty_like(box)
        norms = []
        for k, r in enumerate(roughness):
            o, nk = _cube_level(n, ct, k)
            if r == 0:
                packed[:, o:o + nk * nk * ct] = box[:, o:o + nk * nk * ct]
                norms.append(None)
                continue
            norms.append(torch.empty((6, nk, nk), dtype=torch.float32, device=dev))
            _envmap_filter(box[0, o:], packed[0, o:], floats, norms[-1], nk, ct, r * r, _lib.ENVMAP_GGX)
        ctx.save_for_backward(*[x for x in norms if x is not None])
        ctx.meta = (n, ct, levels, floats, roughness)
        return packed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_packed):
        n, ct, levels, floats, roughness = ctx.meta
        norms = iter(ctx.saved_tensors)
        grad_packed = grad_packed.to(torch.float32).contiguous()
        dev = grad_packed.device
        grad_box = torch.empty_like(grad_packed)       # every level is fully written
        for k, r in enumerate(roughness):
            o, nk = _cube_level(n, ct, k)
            if r == 0:
                grad_box[:, o:o + nk * nk * ct] = grad_packed[:, o:o + nk * nk * ct]
                continue
            _envmap_filter(grad_packed[0, o:], grad_box[0, o:], floats, next(norms), nk, ct, r * r, _lib.ENVMAP_GGX, transposed=True)
        grad_cube = torch.empty((6, n, n, ct), dtype=torch.float32, device=dev)
        _call_entry('mip_collapse', 6, dev, (grad_box.data_ptr(), grad_cube.data_ptr()), n, n, ct, levels)
        return grad_cube, None, None, None


def prefilter_cube(cube, roughness=None, *, max_level=None):
    """The GGX-prefiltered pyramid of an environment cube [6, N, N, C] (the specular half of split-sum image-based lighting) as a
    `CubePyramid`: the box pyramid per face (`cube_pyramid`, with its level count and layout), level k then convolved with a GGX
    lobe of roughness[k] as `convolve_cube` does.  `roughness`: a float per level, each 0 or in [1/32, 1]; default k / (L - 1)
    for L levels, so that `sample_cube_pyramid(pyramid, directions, roughness * (L - 1))` reads a reflection of that roughness.
    Differentiable with respect to the cube (the transposed convolution of every level, then the pyramid's collapse); the same
    bits on every run."""
    who = 'prefilter_cube'
    n, ct, levels, floats = _pyramid_geometry(cube, max_level, who)
    if roughness is None:
        roughness = tuple(k / (levels - 1) for k in range(levels)) if levels > 1 else (0.0,)
    if isinstance(roughness, torch.Tensor) or not isinstance(roughness, (tuple, list)) or len(roughness) != levels:
        raise ValueError('%s: roughness must be a tuple of %d floats, one per level, got %r' % (who, levels, roughness))
    roughness = tuple(_check_roughness(r, who) for r in roughness)
    _stage.require_gpu(cube, 'dirt_amd.texture.prefilter_cube')
    return CubePyramid(_PrefilterCube.apply(cube.to(torch.float32), roughness, levels, floats), n, ct, levels, roughness)


class _SampleCubePyramid(torch.autograd.Function):
    """packed [6, floats], directions [..., 3], lod [...]: `_SampleTextureCube` with the caller's pyramid."""

    @staticmethod
    def forward(ctx, packed, directions, lod, lod_bias, n, ct, levels):
        pyr = packed.contiguous()
        src, stride = _stage.rows_in_place(directions, 3)
        rows, cols, _ = _pixel_grid(directions.shape)
        lod_t = lod.to(torch.float32).contiguous()
        out = torch.empty(tuple(directions.shape[:-1]) + (ct,), dtype=torch.float32, device=pyr.device)
        _call(_lib.load().dirt_texture_cube_forward, pyr.device, pyr.data_ptr(), _stage.ptr(src), _stage.ptr(lod_t), _stage.ptr(out), rows * cols, n, ct,
              levels, stride, lod_bias, 0)
        ctx.save_for_backward(pyr, src, lod_t)
        ctx.meta = (stride, lod_bias, tuple(directions.shape), rows, cols, n, ct, levels)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pyr, src, lod_t = ctx.saved_tensors
        stride, lod_bias, dir_shape, rows, cols, n, ct, levels = ctx.meta
        dev = pyr.device
        grad_out = grad_out.contiguous().to(torch.float32)
        grad_pyr = torch.empty_like(pyr)               # cleared by the call
        grad_dirs = torch.empty(dir_shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        grad_lod = torch.empty(dir_shape[:-1], dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        _call(_lib.load().dirt_texture_cube_backward, dev, pyr.data_ptr(), _stage.ptr(src), _stage.ptr(lod_t), _stage.ptr(grad_out), grad_pyr.data_ptr(),
              _stage.ptr(grad_dirs), _stage.ptr(grad_lod), rows, cols, n, ct, levels, stride, 3, lod_bias, 0)
        return grad_pyr, grad_dirs, grad_lod, None, None, None, None


def sample_cube_pyramid(pyramid, directions, lod, *, lod_bias=0.0):
    """The trilinear look-up of `sample_texture_cube` in a pyramid the caller made (`cube_pyramid`, `prefilter_cube`): directions
    [..., 3] and lod shaped like directions[..., 0] -> [..., C], two adjacent levels blended at the level of detail `lod` +
    `lod_bias`.  The pyramid is not rebuilt: the same kernels read `pyramid.packed`.  Differentiable with respect to
    `pyramid.packed` (and through it the cube), the directions and lod."""
    who = 'sample_cube_pyramid'
    if not isinstance(pyramid, CubePyramid):
        raise ValueError('%s expects a CubePyramid (cube_pyramid, prefilter_cube), got %s' % (who, type(pyramid).__name__))
    packed = pyramid.packed
    if not isinstance(directions, torch.Tensor) or directions.dim() < 1 or directions.shape[-1] != 3:
        raise ValueError('%s expects directions of shape [..., 3], got %s' % (who, tuple(getattr(directions, 'shape', ()))))
    if not directions.is_floating_point():
        raise ValueError('%s: directions must be a floating-point tensor, got %s' % (who, directions.dtype))
    if packed.device != directions.device:
        raise ValueError('pyramid and directions must be on the same device (%s vs %s)' % (packed.device, directions.device))
    if not isinstance(lod, torch.Tensor) or tuple(lod.shape) != tuple(directions.shape[:-1]):
        raise ValueError('lod must be a tensor shaped like directions[..., 0] %s, got %s' % (tuple(directions.shape[:-1]), tuple(getattr(lod, 'shape', ()))))
    if lod.device != directions.device:
        raise ValueError('lod and directions must be on the same device (%s vs %s)' % (lod.device, directions.device))
    _stage.require_gpu(packed, 'dirt_amd.texture.sample_cube_pyramid')
    return _SampleCubePyramid.apply(packed, directions.to(torch.float32), lod, float(lod_bias), pyramid.size, pyramid.channels, pyramid.levels)


# ---- lat-long (equirectangular) panoramas: the environment as it is captured (dirt_panorama.hip; specification in DESIGN.md §7k) ------

_K2, _K1 = 1. / (2. * math.pi), 1. / math.pi   # phi -> u and theta -> v are products with these, rounded to the tensor's dtype


def _check_count(who, name, value, most=None):
    if isinstance(value, bool) or not isinstance(value, int) or value < 1 or (most is not None and value > most):
        raise ValueError('%s: %s must be %s, got %r' % (who, name, 'a positive int' if most is None else 'an int in 1..%d' % most, value))


def panorama_texel_directions(height, width, samples=1, device=None, dtype=torch.float32):
    """-> (directions [height * samples, width * samples, 3], unit vectors through the centres of the samples x samples
    sub-samples of a panorama's pixels, and weights [height * samples, width * samples], their solid angles up to a constant:
    sin theta).  Row 0 is +Y, the middle column looks along -Z, columns grow towards +X.  The inverse of
    `directions_to_panorama_indices`: with samples = 1, direction [i, j] maps back to index (i, j).  Pure torch."""
    who = 'panorama_texel_directions'
    _check_count(who, 'height', height)
    _check_count(who, 'width', width)
    _check_count(who, 'samples', samples, _lib.PANORAMA_MAX_SAMPLES)

    def centres(n):
        k = torch.arange(n * samples, device=device)
        return (torch.div(k, samples, rounding_mode='floor').to(dtype) + ((k % samples).to(dtype) + 0.5) / samples) / n

    theta, phi = math.pi * centres(height)[:, None], (2. * math.pi) * (centres(width)[None, :] - 0.5)
    st = torch.sin(theta)
    d = torch.stack([st * torch.sin(phi), torch.cos(theta).expand(-1, width * samples), -(st * torch.cos(phi))], -1)
    return d, st.expand(-1, width * samples).contiguous()


def directions_to_panorama_indices(directions, height, width):
    """[..., 3] directions (not normalised) -> (fractional (row, column) indices [..., 2] into a `height` x `width` panorama,
    valid bool [...]): theta = atan2(sqrt(x^2 + z^2), y) from +Y gives the row, theta / pi * height - 0.5 clamped to
    [0, height - 1]; phi = atan2(x, -z) gives the column, (phi / (2 pi) + 0.5) * width - 0.5, which is NOT wrapped here (it lies
    in [-0.5, width - 0.5]; `sample_panorama` wraps its taps).  Straight up or down (x = z = 0) takes phi = 0 and no gradient.
    The length of a direction does not matter, at either end of the dtype's range: (x, y, z) is the direction times the exact
    power of two that brings its largest component into [0.5, 1) (`frexp`; a subnormal component included), so x^2 + z^2 neither
    overflows nor underflows, and the gradient is scaled back by the same power of two.
    A direction that is not finite or is all zero is not valid: index 0, and no gradient.  Pure torch, on any device,
    differentiable; `sample_panorama(panorama, *directions_to_panorama_indices(directions, H, W))` is a panorama's look-up."""
    who = 'directions_to_panorama_indices'
    if not isinstance(directions, torch.Tensor) or directions.dim() < 1 or directions.shape[-1] != 3 or not directions.is_floating_point():
        raise ValueError('%s expects floating-point directions of shape [..., 3], got %s' % (who, tuple(getattr(directions, 'shape', ()))))
    _check_count(who, 'height', height)
    _check_count(who, 'width', width)
    with torch.no_grad():
        valid = torch.isfinite(directions).all(-1) & (directions.abs().amax(-1) > 0)
    up = torch.zeros_like(directions)
    up[..., 1] = 1.
    d = torch.where(valid.unsqueeze(-1), directions, up)
    with torch.no_grad():   # 2^-e, e the exponent of the largest component: exact, and in two factors (2^148 is no float32)
        e = torch.frexp(d.abs().amax(-1, keepdim=True))[1]
        half = torch.div(-e, 2, rounding_mode='floor')
        one = torch.ones_like(d[..., :1])
        s1, s2 = torch.ldexp(one, half), torch.ldexp(one, -e - half)
    x, y, z = ((d * s1) * s2).unbind(-1)
    rho2 = x * x + z * z
    with torch.no_grad():
        pole = rho2.sqrt() == 0
    one = torch.ones_like(rho2)
    rho = torch.where(pole, torch.zeros_like(rho2), torch.where(pole, one, rho2).sqrt())
    theta = torch.atan2(rho, y)
    phi = torch.where(pole, torch.zeros_like(rho2), torch.atan2(torch.where(pole, one, x), -torch.where(pole, one, z)))
    col = (phi * _K2 + 0.5) * float(width) - 0.5
    row = ((theta * _K1) * float(height) - 0.5).clamp(0., float(height - 1))
    indices = torch.stack([row, col], -1)
    return torch.where(valid.unsqueeze(-1), indices, torch.zeros_like(indices)), valid


def sample_panorama(panorama, indices, valid):
    """panorama [H, W, C], and per look-up the fractional (row, column) `indices` [..., 2] and `valid` of
    `directions_to_panorama_indices` -> [..., C]: the bilinear blend of the four texels around the index, columns wrapping
    around the panorama and rows clamped to it; 0 where not valid.  Pure torch, differentiable."""
    h, w = int(panorama.shape[0]), int(panorama.shape[1])
    floor = torch.floor(indices)
    frac = indices - floor
    r, c = floor[..., 0].to(torch.int64).clamp(0, h - 1), torch.remainder(floor[..., 1].to(torch.int64), w)
    r1, c1 = (r + 1).clamp(max=h - 1), torch.remainder(c + 1, w)
    fr, fc = frac[..., :1], frac[..., 1:]
    out = (panorama[r, c] * (1. - fc) * (1. - fr) + panorama[r, c1] * fc * (1. - fr)) + panorama[r1, c] * (1. - fc) * fr + panorama[r1, c1] * fc * fr
    return torch.where(valid.unsqueeze(-1), out, torch.zeros_like(out))


def _box_mean(x, samples):
    """[..., R * S, C * S, ch] -> [..., R, C, ch]: the S x S samples of a texel added in row-major order, then times 1 / S^2."""
    acc = None
    for a in range(samples):
        for b in range(samples):
            s = x[..., a::samples, b::samples, :]
            acc = s if acc is None else acc + s
    return acc * (1. / (samples * samples))


def _check_panorama_arguments(who, source, what, shape_text, rotation, samples, **counts):
    """The checks `panorama_to_cube` and `cube_to_panorama` share with their dense forms -> the rotation as a tensor (None: the
    identity)."""
    ok = isinstance(source, torch.Tensor) and 0 not in source.shape and (
        source.dim() == 3 if what == 'panorama' else source.dim() == 4 and source.shape[0] == 6 and source.shape[1] == source.shape[2])
    if not ok:
        raise ValueError('%s expects %s to be %s, got %s' % (who, what, shape_text, tuple(source.shape) if isinstance(source, torch.Tensor) else type(source).__name__))
    if not source.is_floating_point():
        raise ValueError('%s: %s must be a floating-point tensor, got %s' % (who, what, source.dtype))
    for name, value in counts.items():
        _check_count(who, name, value)
    _check_count(who, 'samples', samples, _lib.PANORAMA_MAX_SAMPLES)
    if rotation is None:
        return torch.eye(3, dtype=source.dtype, device=source.device)
    if not isinstance(rotation, torch.Tensor) or tuple(rotation.shape) != (3, 3) or not rotation.is_floating_point():
        raise ValueError('%s: rotation must be a floating-point tensor [3, 3] or None, got %s' % (
            who, '%s %s' % (rotation.dtype, tuple(rotation.shape)) if isinstance(rotation, torch.Tensor) else type(rotation).__name__))
    if rotation.device != source.device:
        raise ValueError('%s: rotation is on %s, the %s on %s' % (who, rotation.device, what, source.device))
    return rotation


def _cube_sample_directions(size, samples, device, dtype):
    """The directions (not normalised) through the samples x samples sub-samples of a cube's texels [6, size * samples,
    size * samples, 3], by the table of `cube_texel_directions`."""
    k = torch.arange(size * samples, device=device)
    x = (2. * (torch.div(k, samples, rounding_mode='floor').to(dtype) + ((k % samples).to(dtype) + 0.5) / samples)) / size - 1.
    tc, sc = torch.meshgrid(x, x, indexing='ij')
    one = torch.ones_like(sc)
    return torch.stack([torch.stack(f, -1) for f in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one))])


def _rotate(d, rotation, transposed):
    """d @ rotation (or @ rotation^T) with the three products added in order, as the kernels add them"""
    m = rotation.t() if transposed else rotation
    return (d[..., 0:1] * m[0] + d[..., 1:2] * m[1]) + d[..., 2:3] * m[2]


def panorama_to_cube_dense(panorama, size, samples=1, rotation=None):
    """The specification of `panorama_to_cube`: pure torch, on any device, in the panorama's dtype, differentiable with respect
    to the panorama and the rotation.  panorama [H, W, C] (row 0 at +Y, the middle column along -Z, columns growing towards
    +X) -> cube [6, size, size, C]: every texel the mean of samples x samples look-ups (`sample_panorama`) at
    e @ rotation^T, e the directions through the sub-samples' places on the face.  `rotation` [3, 3] in row vectors: its
    rows are the images of the panorama's axes in the cube's frame; None is the identity."""
    who = 'panorama_to_cube_dense'
    rotation = _check_panorama_arguments(who, panorama, 'panorama', '3D [height, width, channels]', rotation, samples, size=size)
    e = _cube_sample_directions(size, samples, panorama.device, panorama.dtype)
    h, w = int(panorama.shape[0]), int(panorama.shape[1])
    looked = sample_panorama(panorama, *directions_to_panorama_indices(_rotate(e, rotation.to(panorama.dtype), True), h, w))
    return _box_mean(looked, samples)


def cube_to_panorama_dense(cube, height, width, samples=1, rotation=None):
    """The specification of `cube_to_panorama`: pure torch, differentiable with respect to the cube and the rotation.  cube
    [6, N, N, C] -> panorama [height, width, C]: every pixel the mean of samples x samples bilinear cube look-ups
    (`directions_to_cube_indices`, `sample_cube`) at d @ rotation, d the sub-samples' `panorama_texel_directions`."""
    who = 'cube_to_panorama_dense'
    rotation = _check_panorama_arguments(who, cube, 'cube', '4D [6, size, size, channels]', rotation, samples, height=height, width=width)
    d, _ = panorama_texel_directions(height, width, samples, cube.device, cube.dtype)
    looked = sample_cube(cube, *directions_to_cube_indices(_rotate(d, rotation.to(cube.dtype), False), int(cube.shape[1])))
    return _box_mean(looked, samples)


class _PanoramaResample(torch.autograd.Function):
    """source [H, W, C] -> [6, size, size, C] (`to_cube`), or source [6, N, N, C] -> [height, width, C]; rotation [3, 3]."""

    @staticmethod
    def forward(ctx, source, rotation, to_cube, rows, cols, size, samples):
        source, rotation = source.contiguous(), rotation.contiguous()
        ct = int(source.shape[-1])
        lib = _lib.load()
        out = torch.empty((6, size, size, ct) if to_cube else (rows, cols, ct), dtype=torch.float32, device=source.device)
        _call(lib.dirt_panorama_to_cube_forward if to_cube else lib.dirt_cube_to_panorama_forward, source.device, source.data_ptr(), rotation.data_ptr(),
              out.data_ptr(), rows, cols, size, ct, samples)
        ctx.save_for_backward(source, rotation)
        ctx.meta = (to_cube, rows, cols, size, ct, samples)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        source, rotation = ctx.saved_tensors
        to_cube, rows, cols, size, ct, samples = ctx.meta
        lib, dev = _lib.load(), source.device
        grad_out = grad_out.contiguous().to(torch.float32)
        grad_source = torch.empty_like(source) if ctx.needs_input_grad[0] else None
        grad_rotation = torch.empty_like(rotation) if ctx.needs_input_grad[1] else None
        need = to_cube and grad_rotation is not None or not to_cube and (grad_source is not None or grad_rotation is not None)
        nbytes = lib.dirt_panorama_scratch_bytes(rows, cols, size, ct, samples, int(to_cube)) if need else 0
        scratch = _stage.scratch(dev, nbytes)
        _call(lib.dirt_panorama_to_cube_backward if to_cube else lib.dirt_cube_to_panorama_backward, dev, source.data_ptr(), rotation.data_ptr(),
              grad_out.data_ptr(), _stage.ptr(grad_source), _stage.ptr(grad_rotation), _stage.ptr(scratch), nbytes, rows, cols, size, ct, samples)
        return grad_source, grad_rotation, None, None, None, None, None


def panorama_to_cube(panorama, size, *, samples=1, rotation=None):
    """Fused `panorama_to_cube_dense`: a lat-long (equirectangular) panorama [H, W, C] float32 -- row 0 at +Y, the middle column
    along -Z, columns growing towards +X -- resampled into a cube [6, size, size, C] (faces in OpenGL order), what
    `prefilter_cube`, `shade_gbuffer_ibl` and `environment_background` take.  Every texel is the mean of samples x samples
    (1..4) bilinear look-ups of the panorama, whose columns wrap and whose rows clamp.  `rotation` [3, 3] in row vectors turns
    the panorama: its rows are the images of the panorama's axes in the cube's frame (`matrices.rodrigues(w,
    three_by_three=True)`); None is the identity, to the bit.  It need be no rotation, and its scale does not matter: a look-up
    scales its direction by an exact power of two first (`directions_to_panorama_indices`), subnormal directions included, so
    2^k times a matrix gives the same cube to the bit.  Differentiable with respect to the panorama (float atomics) and the
    rotation (the same bits on every run)."""
    who = 'panorama_to_cube'
    rotation = _check_panorama_arguments(who, panorama, 'panorama', '3D [height, width, channels]', rotation, samples, size=size)
    _stage.require_gpu(panorama, 'dirt_amd.texture.panorama_to_cube')
    return _PanoramaResample.apply(panorama.to(torch.float32), rotation.to(torch.float32), True, int(panorama.shape[0]), int(panorama.shape[1]),
                                   size, samples)


def cube_to_panorama(cube, height, width, *, samples=1, rotation=None):
    """Fused `cube_to_panorama_dense`: a cube [6, N, N, C] float32 resampled into a lat-long panorama [height, width, C], the
    inverse of `panorama_to_cube` up to the two resamplings.  Every pixel is the mean of samples x samples (1..4) bilinear cube
    look-ups (`sample_texture_cube`'s) at d @ rotation, d the directions of the sub-samples; `rotation` as in
    `panorama_to_cube` (the same matrix takes a panorama to the cube and back).  Differentiable with respect to the cube (float
    atomics) and the rotation (the same bits on every run)."""
    who = 'cube_to_panorama'
    rotation = _check_panorama_arguments(who, cube, 'cube', '4D [6, size, size, channels]', rotation, samples, height=height, width=width)
    _stage.require_gpu(cube, 'dirt_amd.texture.cube_to_panorama')
    return _PanoramaResample.apply(cube.to(torch.float32), rotation.to(torch.float32), False, height, width, int(cube.shape[1]), samples)
