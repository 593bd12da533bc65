"""Fused G-buffer lighting for deferred shaders: the shader of the reference's samples/deferred.py:59-98 (ambient + the
reflectance models of dirt/lighting.py:175-344, composited over a background colour through the mask channel, clamped)
as one HIP kernel forward and one backward (dirt_shade.hip; specification in DESIGN.md §7b).

`shade_gbuffer` is usable directly and as the body of a `shader_fn` given to `rasterise_deferred`:

    def shader_fn(gbuffer, view_matrix, light_direction):
        return shade_gbuffer(gbuffer, [diffuse_directional_light(light_direction, (1., 0., 0.), double_sided=False)],
                             colors=4, normals=7, positions=1, mask=0, ambient=(.2, .2, .2), background=(0., 0., .3))

`colors` may also be a tensor [..., 3] beside the G-buffer -- the output of `texture.sample_texture_uv`, of a network -- which
the same kernels read in place of the three channels and whose gradient they write (examples/textured_fused.py).
"""
import math
import numbers

import torch

from . import _lib
from . import _stage
from ._stage import ptr as _ptr

_KINDS = _lib.SHADE_KINDS
_NEEDS_POSITIONS = ('specular_directional', 'diffuse_point')


def diffuse_directional_light(direction, color, double_sided=True):
    """A light record for `shade_gbuffer`: `lighting.diffuse_directional` (dirt/lighting.py:175-218)."""
    return ('diffuse_directional', direction, color, double_sided)


def specular_directional_light(direction, color, shininess, double_sided=True):
    """A light record for `shade_gbuffer`: `lighting.specular_directional` (dirt/lighting.py:221-283); needs `camera_position`."""
    return ('specular_directional', direction, color, shininess, double_sided)


def diffuse_point_light(position, color, double_sided=True):
    """A light record for `shade_gbuffer`: `lighting.diffuse_point` (dirt/lighting.py:286-344)."""
    return ('diffuse_point', position, color, double_sided)


# (device, values) -> [1, P] tensor of the block's constant part, uploaded once per distinct set of python numbers.  Rows are
# NEVER evicted: a captured HIP graph (GraphedStep) replays from the address of the row its warm-up allocated, and nothing else
# keeps that row alive once the call has returned.  A row is at most 292 bytes; parameters that change from call to call are
# meant to be tensors (which also makes them differentiable), not python numbers.
_const_cache = {}


def _const_block(device, values):
    key = (str(device), values)
    t = _const_cache.get(key)
    if t is None:
        t = _const_cache[key] = torch.tensor([values], dtype=torch.float32).to(device)
    return t


def _value(x, width, name, device, batch):
    """A parameter as python floats (-> list) or as a float32 tensor [1 or batch, width] on `device`."""
    if isinstance(x, torch.Tensor):
        if x.device != device:
            raise ValueError('%s is on %s, the G-buffer on %s' % (name, x.device, device))
        shapes = [(width,), (batch, width)] if batch is not None else [(width,)]
        if width == 1:
            shapes = [(), (1,)] + ([(batch,), (batch, 1)] if batch is not None else [])
        if tuple(x.shape) not in shapes:
            raise ValueError('%s must have shape %s, got %s' % (name, ' or '.join(str(list(s)) for s in shapes), list(x.shape)))
        return x.to(torch.float32).reshape(-1, width)
    if width == 1:
        if not isinstance(x, numbers.Real):
            raise ValueError('%s must be a number or a tensor, got %r' % (name, x))
        return [float(x)]
    try:
        vals = [float(v) for v in x]
    except (TypeError, ValueError):
        raise ValueError('%s must be %d numbers or a tensor, got %r' % (name, width, x))
    if len(vals) != width:
        raise ValueError('%s must be %d numbers, got %d' % (name, width, len(vals)))
    return vals


def _gbuffer_sizes(gbuffer, who):
    """The head of every entry point (`who`): refuses what is no G-buffer by its shape, -> (the G-buffer as a contiguous float32
    tensor -- itself where it is one --, scenes, pixels of a scene, channels)."""
    if not isinstance(gbuffer, torch.Tensor) or gbuffer.dim() not in (2, 3, 4):
        raise ValueError('%s expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got %s' % (who, tuple(getattr(gbuffer, 'shape', ())),))
    batched = gbuffer.dim() == 4
    scenes = int(gbuffer.shape[0]) if batched else 1
    pixels = math.prod(gbuffer.shape[1 if batched else 0:-1]) if scenes else 0
    return gbuffer.to(torch.float32).contiguous(), scenes, pixels, int(gbuffer.shape[-1])


def _param_head(ambient, background, camera_position, dev, batch):
    """The head of a [1 or B, 9 + 8 lights] parameter block as slots (first slot, `_value`): ambient, background, camera."""
    return [(0, _value(ambient, 3, 'ambient', dev, batch)), (3, _value(background, 3, 'background', dev, batch)),
            (6, _value(camera_position, 3, 'camera_position', dev, batch))]


def _split_slots(width, slots):
    """The slots of a parameter block of `width` floats -> (its constant row: the python numbers, zeros elsewhere,
    [(first slot, tensor [1 or B, width])]: what `_splice_block` splices into it)."""
    const, tensors = [0.] * width, []
    for start, v in slots:
        if isinstance(v, list):
            const[start:start + len(v)] = v
        else:
            tensors.append((start, v))
    return const, tensors


def _check_gbuffer(gbuffer, who):
    """What every `_check_*` opens with: refuses a G-buffer that is not floating-point, -> (its device, B of a [B, H, W, Cg] one
    or None)."""
    if not gbuffer.dtype.is_floating_point:
        raise ValueError('%s expects a float32 gbuffer, got %s' % (who, gbuffer.dtype))
    return gbuffer.device, int(gbuffer.shape[0]) if gbuffer.dim() == 4 else None


def _as_input(x):
    """colors / material / a cube as an autograd Function takes it: a tensor as float32, a channel index as None"""
    return x.to(torch.float32) if isinstance(x, torch.Tensor) else None


def _forward_operands(gbuffer, block, colors, material=None):
    """What the lighting forward passes open with: -> (the output [..., 3], the contiguous block, the colour and the material
    tensor beside the G-buffer as they are passed under `_stage.rows_in_place` -- None for channels of the G-buffer --, their
    strides).  (Written out, not looped: this runs in every call.)"""
    out = torch.empty(tuple(gbuffer.shape[:-1]) + (3,), dtype=torch.float32, device=gbuffer.device)
    csrc, cstride = _stage.rows_in_place(colors, 3) if colors is not None else (None, 0)
    msrc, mstride = _stage.rows_in_place(material, 2) if material is not None else (None, 0)
    return out, block.contiguous(), csrc, msrc, cstride, mstride


def _backward_operands(want, grad_out, gbuffer, block, empty, csrc, msrc=None):
    """What the lighting backward passes open with (`want`: the Function's needs_input_grad): -> (the gradients of the G-buffer
    and the block (`_stage.grad_outputs`), of the saved colour and material tensors, inputs 2 and 3 (`_stage.dense_grads`; None,
    not given, wants none), the incoming gradient as the kernels read it -- None for an `empty` call, whose gradients are
    zeroed and complete)."""
    grad_g, grad_p = _stage.grad_outputs((gbuffer, block), want[:2], empty)
    grad_c, grad_m = _stage.dense_grads(grad_out, (3, 2), (csrc is not None and want[2], msrc is not None and want[3]), empty)
    return grad_g, grad_p, grad_c, grad_m, None if empty else grad_out.to(torch.float32).contiguous()


class _ShadeGBuffer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, block, colors, meta):
        """colors: None (three channels of the G-buffer, offsets[0]) or float32 [..., 3] beside it, read in place where its
        pixels lie a constant stride apart (`_stage.rows_in_place`)"""
        lib = _lib.load()
        scenes, pixels, cg, offsets, kinds, sided, nl, lo, hi, flags = meta
        out, block, src, _, stride, _ = _forward_operands(gbuffer, block, colors)
        tail = (int(block.shape[0]), nl, kinds, sided, lo, hi, flags)
        if scenes * pixels and src is None:
            _stage.call(lib.dirt_shade_forward, gbuffer.device, gbuffer.data_ptr(), block.data_ptr(), out.data_ptr(), scenes, pixels, cg,
                        *offsets, *tail)
        elif scenes * pixels:
            _stage.call(lib.dirt_shade_albedo_forward, gbuffer.device, gbuffer.data_ptr(), src.data_ptr(), block.data_ptr(), out.data_ptr(),
                        scenes, pixels, cg, stride, *offsets[1:], *tail)
        ctx.save_for_backward(gbuffer, block, src)
        ctx.meta, ctx.color_stride = meta, stride
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, block, src = ctx.saved_tensors
        scenes, pixels, cg, offsets, kinds, sided, nl, lo, hi, flags = ctx.meta
        dev = gbuffer.device
        grad_g, grad_p, grad_c, _, grad_out = _backward_operands(ctx.needs_input_grad, grad_out, gbuffer, block, not scenes * pixels, src)
        if grad_out is None:
            return grad_g, grad_p, grad_c, None
        nbytes = lib.dirt_shade_scratch_bytes(scenes, pixels, nl) if grad_p is not None else 0
        tail = (_ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, pixels, cg)
        if src is None:
            _stage.call(lib.dirt_shade_backward, dev, gbuffer.data_ptr(), block.data_ptr(), grad_out.data_ptr(), _ptr(grad_g), _ptr(grad_p),
                        *tail, *offsets, int(block.shape[0]), nl, kinds, sided, lo, hi, flags)
        else:
            _stage.call(lib.dirt_shade_albedo_backward, dev, gbuffer.data_ptr(), src.data_ptr(), block.data_ptr(), grad_out.data_ptr(),
                        _ptr(grad_g), _ptr(grad_c), _ptr(grad_p), *tail, ctx.color_stride, *offsets[1:], int(block.shape[0]), nl, kinds, sided,
                        lo, hi, flags)
        return grad_g, grad_p, grad_c, None


def shade_gbuffer(gbuffer, lights, *, colors, normals, positions=None, mask=None, ambient=(0., 0., 0.), camera_position=None,
                  background=(0., 0., 0.), clamp=(0., 1.)):
    """Lights a G-buffer per pixel in one kernel (the shader of samples/deferred.py:59-98), differentiably.

    gbuffer: float32 [H, W, Cg], [B, H, W, Cg] or a flat [N, Cg] on the GPU; a contiguous one is read in place.
    colors, normals, positions, mask: the first channel of each attribute inside a pixel (3, 3, 3 and 1 channels; any
        order, no overlap).  `positions` is needed only if a light needs it; mask=None: every pixel is covered.
    colors may instead be a floating-point tensor shaped like the G-buffer with 3 channels ([H, W, 3], [B, H, W, 3], [N, 3])
        on its device: the colours come from it, it is differentiable, and the G-buffer needs no colour channels (normals,
        positions and mask may sit anywhere).  One whose pixels lie a constant stride >= 3 floats apart -- a contiguous
        tensor, the first or last three channels of an RGBA image, `gbuffer[..., 4:7]` -- is read in place.
    lights: up to 8 records ('diffuse_directional', direction, color, double_sided),
        ('specular_directional', direction, color, shininess, double_sided) (needs `camera_position`) or
        ('diffuse_point', position, color, double_sided) -- the three models of `dirt_amd.lighting`, with their conventions
        (nothing is renormalised); `diffuse_directional_light` etc. build them.
    direction / position / color / ambient / camera_position / background: 3 numbers or a tensor [3], or [B, 3] with a
        [B, H, W, Cg] G-buffer (one value per scene); shininess: a number, a 0-d tensor or [B].  Tensors must be on the
        G-buffer's device, stay there (no host synchronisation: the call can be captured in a HIP graph) and are differentiable.
    clamp: (lo, hi) or None.

    Returns [..., 3]:  clamp(lit * m + background * (1 - m), lo, hi)  with  lit = ambient * c + sum of the lights' terms,
    each what the function of the same name in `dirt_amd.lighting` returns with vertex_colors = vertex_reflectivities = c.
    Gradients are those of torch's autograd for that composition, including at the kinks (max(x, 0) and clamp pass the
    gradient at their edges, abs gives 0 at 0).  A shininess below 1 at a zero cosine (0 * inf in torch) is not defined."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'shade_gbuffer')
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.shade_gbuffer')
    lights = list(lights)
    offsets, kinds, sided, lo, hi, flags, const, tensors = _check_arguments(gbuffer, lights, colors, normals, positions, mask, ambient,
                                                                            camera_position, background, clamp)
    block = _splice_block(gbuffer.device, const, tensors)
    meta = (scenes, pixels, cg, tuple(offsets), kinds, sided, len(lights), lo, hi, flags)
    return _ShadeGBuffer.apply(g, block, _as_input(colors), meta)


def _splice_block(dev, const, tensors):
    """The parameter block [1 or B, len(const)]: the cached constant row with the tensors spliced in by one torch.cat, whose
    autograd hands the block's gradient back to them (and drops the constant part's)."""
    block, width = _const_block(dev, tuple(const)), len(const)
    if tensors:
        rows = max(int(t.shape[0]) for _, t in tensors)
        pieces, cursor = [], 0
        for start, t in sorted(tensors, key=lambda st: st[0]):
            if start > cursor:
                pieces.append(block[:, cursor:start].expand(rows, -1))
            pieces.append(t.expand(rows, -1))
            cursor = start + int(t.shape[1])
        if cursor < width:
            pieces.append(block[:, cursor:].expand(rows, -1))
        block = torch.cat(pieces, dim=1)
    return block


def _check_arguments(gbuffer, lights, colors, normals, positions, mask, ambient, camera_position, background, clamp):
    """Everything `shade_gbuffer` refuses with a ValueError, on the tensor's shape and device alone (no device work): ->
    (channel offsets, light kinds, sidedness, lo, hi, flags, the block's constant row, [(first slot, tensor [1 or B, width])]).
    `colors` as a tensor: the offsets' first entry is -1."""
    dev, batch = _check_gbuffer(gbuffer, 'shade_gbuffer')
    offsets = _channel_offsets(gbuffer, (('colors', colors, 3, True), ('normals', normals, 3, True), ('positions', positions, 3, False),
                                         ('mask', mask, 1, False)))
    if len(lights) > _lib.SHADE_MAX_LIGHTS:
        raise ValueError('shade_gbuffer takes at most %d lights, got %d' % (_lib.SHADE_MAX_LIGHTS, len(lights)))
    lo, hi = _clamp_bounds(clamp)
    flags = (_lib.SHADE_CLAMP if clamp is not None else 0) | (_lib.SHADE_HAS_CAMERA if camera_position is not None else 0)
    kinds, sided, const, tensors = _light_block(lights, positions, ambient, camera_position, background, dev, batch)
    return offsets, kinds, sided, lo, hi, flags, const, tensors


def _channel_offsets(gbuffer, attributes):
    """The first channel of each of `attributes` (name, channel index or None or -- colors and material only -- a tensor, width,
    required) inside a pixel of `gbuffer`, -1 for an absent one and for one that is a tensor; refuses what does not fit or overlaps."""
    dev = gbuffer.device
    cg = int(gbuffer.shape[-1])
    offsets, offsets_named = [], []
    for name, off, width, required in attributes:
        if off is None and not required:
            offsets.append(-1)
            continue
        if name in ('colors', 'material') and isinstance(off, torch.Tensor):
            want = tuple(gbuffer.shape[:-1]) + (width,)
            if not off.dtype.is_floating_point:
                raise ValueError('%s as a tensor must be floating-point, got %s' % (name, off.dtype))
            if tuple(off.shape) != want:
                raise ValueError('%s as a tensor must have shape %s (the G-buffer\'s %s with %d channels), got %s'
                                 % (name, list(want), list(gbuffer.shape), width, list(off.shape)))
            if off.device != dev:
                raise ValueError('%s is on %s, the G-buffer on %s' % (name, off.device, dev))
            offsets.append(-1)
            continue
        if isinstance(off, bool) or not isinstance(off, int):
            raise ValueError('%s must be the index of a G-buffer channel, got %r' % (name, off))
        if off < 0 or off + width > cg:
            raise ValueError('%s at channel %d does not fit in the %d channels of the G-buffer' % (name, off, cg))
        for other, o, w in offsets_named:
            if off < o + w and o < off + width:
                raise ValueError('%s (channel %d) overlaps %s (channel %d)' % (name, off, other, o))
        offsets_named.append((name, off, width))
        offsets.append(off)
    return offsets


def _clamp_bounds(clamp):
    """(lo, hi) of `clamp`, (0, 0) for None"""
    if clamp is None:
        return 0., 0.
    try:
        lo, hi = (float(v) for v in clamp)
    except (TypeError, ValueError):
        raise ValueError('clamp must be (lo, hi) or None, got %r' % (clamp,))
    if not lo <= hi:
        raise ValueError('clamp needs lo <= hi, got %r' % (clamp,))
    return lo, hi


def _light_block(lights, positions, ambient, camera_position, background, dev, batch):
    """The parameter block of `shade_gbuffer` -> (light kinds, sidedness, its constant row, [(first slot, tensor [1 or B, width])])."""
    # the parameter block: [1 or B, 9 + 8 lights]; python numbers go into a cached constant row, tensors are spliced in with
    # one torch.cat whose autograd hands the block's gradient back to them
    slots = _param_head(ambient, background, camera_position if camera_position is not None else (0., 0., 0.), dev, batch)
    kinds = sided = 0
    for l, rec in enumerate(lights):
        if not isinstance(rec, (tuple, list)) or not rec or rec[0] not in _KINDS:
            raise ValueError('light %d: expected a record starting with one of %s, got %r' % (l, sorted(_KINDS), rec))
        kind = rec[0]
        if len(rec) != (5 if kind == 'specular_directional' else 4):
            raise ValueError('light %d: a %s record has %d fields, got %d' % (l, kind, 5 if kind == 'specular_directional' else 4, len(rec)))
        if kind in _NEEDS_POSITIONS and positions is None:
            raise ValueError('light %d (%s) needs the `positions` channels of the G-buffer' % (l, kind))
        if kind == 'specular_directional' and camera_position is None:
            raise ValueError('light %d (specular_directional) needs camera_position' % l)
        base = _lib.SHADE_PARAM_HEAD + _lib.SHADE_PARAM_LIGHT * l
        slots.append((base, _value(rec[1], 3, 'light %d %s' % (l, 'position' if kind == 'diffuse_point' else 'direction'), dev, batch)))
        slots.append((base + 3, _value(rec[2], 3, 'light %d color' % l, dev, batch)))
        if kind == 'specular_directional':
            slots.append((base + 6, _value(rec[3], 1, 'light %d shininess' % l, dev, batch)))
        kinds |= _KINDS[kind] << (2 * l)
        sided |= (1 if rec[-1] else 0) << l
    return (kinds, sided) + _split_slots(_lib.SHADE_PARAM_HEAD + _lib.SHADE_PARAM_LIGHT * len(lights), slots)


# ---- spherical-harmonic lighting (dirt_shade_sh.hip)

_SH_TERMS = 9


class _ShadeGBufferSH(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, block, colors, meta):
        """colors: None (three channels of the G-buffer) or float32 [..., 3] beside it, read in place under `_stage.rows_in_place`"""
        lib = _lib.load()
        scenes, pixels, cg, offsets, scale, lo, hi, flags = meta
        out, block, src, _, stride, _ = _forward_operands(gbuffer, block, colors)
        if scenes * pixels:
            _stage.call(lib.dirt_shade_sh_forward, gbuffer.device, gbuffer.data_ptr(), _ptr(src), block.data_ptr(), out.data_ptr(), scenes, pixels,
                        cg, stride, *offsets, int(block.shape[0]), *scale, lo, hi, flags)
        ctx.save_for_backward(gbuffer, block, src)
        ctx.meta, ctx.color_stride = meta, stride
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, block, src = ctx.saved_tensors
        scenes, pixels, cg, offsets, scale, lo, hi, flags = ctx.meta
        dev = gbuffer.device
        grad_g, grad_p, grad_c, _, grad_out = _backward_operands(ctx.needs_input_grad, grad_out, gbuffer, block, not scenes * pixels, src)
        if grad_out is None:
            return grad_g, grad_p, grad_c, None
        nbytes = lib.dirt_shade_sh_scratch_bytes(scenes, pixels) if grad_p is not None else 0
        _stage.call(lib.dirt_shade_sh_backward, dev, gbuffer.data_ptr(), _ptr(src), block.data_ptr(), grad_out.data_ptr(), _ptr(grad_g),
                    _ptr(grad_c), _ptr(grad_p), _ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, pixels, cg, ctx.color_stride, *offsets,
                    int(block.shape[0]), *scale, lo, hi, flags)
        return grad_g, grad_p, grad_c, None


def shade_gbuffer_sh(gbuffer, coefficients, *, colors, normals, mask=None, background=(0., 0., 0.), clamp=(0., 1.), normalize=False,
                     band_scale=(1., 1., 1.)):
    """Lights a G-buffer per pixel with second-order spherical harmonics in one kernel, differentiably: what
    `lighting.spherical_harmonics` computes per vertex, composited and clamped as `shade_gbuffer` does.

    gbuffer, colors (channel index or tensor [..., 3]), normals, mask, background, clamp: as in `shade_gbuffer`.
    coefficients: a floating-point tensor [K, 3], or [B, K, 3] with a [B, H, W, Cg] G-buffer (one table per scene), K in
        (1, 4, 9): bands 0, 0-1 or 0-2 in the order of `lighting.sh_basis`, one column per colour channel.  On the G-buffer's
        device, differentiable.
    normalize: the normals go through torch.nn.functional.normalize (n / max(|n|, 1e-12)) first, with its gradient;
        otherwise they are taken as given.
    band_scale: three python numbers multiplying bands 0, 1, 2 (`lighting.SH_LAMBERT`: radiance -> irradiance); not differentiable.

    Returns [..., 3]:  clamp(c * E * m + background * (1 - m), lo, hi)  with  E_j = sum_k band_scale[band(k)] L[k, j] Y_k(n).
    Gradients are those of torch's autograd for that composition (the clamp passes the gradient at its edges)."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'shade_gbuffer_sh')
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.shade_gbuffer_sh')
    offsets, scale, lo, hi, flags, const, tensors = _check_sh_arguments(gbuffer, coefficients, colors, normals, mask, background, clamp,
                                                                        normalize, band_scale)
    block = _splice_block(gbuffer.device, const, tensors)
    meta = (scenes, pixels, cg, tuple(offsets), scale, lo, hi, flags)
    return _ShadeGBufferSH.apply(g, block, _as_input(colors), meta)


def _check_sh_arguments(gbuffer, coefficients, colors, normals, mask, background, clamp, normalize, band_scale):
    """Everything `shade_gbuffer_sh` refuses with a ValueError, on shapes and devices alone (no device work): -> (channel
    offsets (colors, normals, mask), band scales, lo, hi, flags, the block's constant row, [(first slot, tensor [1 or B, width])])."""
    dev, batch = _check_gbuffer(gbuffer, 'shade_gbuffer_sh')
    offsets = _channel_offsets(gbuffer, (('colors', colors, 3, True), ('normals', normals, 3, True), ('mask', mask, 1, False)))
    if not isinstance(coefficients, torch.Tensor) or not coefficients.dtype.is_floating_point:
        raise ValueError('coefficients must be a floating-point tensor, got %s' % (getattr(coefficients, 'dtype', type(coefficients).__name__),))
    shape = tuple(coefficients.shape)
    if len(shape) not in (2, 3) or shape[-1] != 3 or shape[-2] not in (1, 4, 9):
        raise ValueError('coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got %s' % list(shape))
    if len(shape) == 3 and shape[0] != batch:
        raise ValueError('coefficients [B, K, 3] need a [B, H, W, Cg] G-buffer with the same B, got %s against a G-buffer %s'
                         % (list(shape), list(gbuffer.shape)))
    if coefficients.device != dev:
        raise ValueError('coefficients is on %s, the G-buffer on %s' % (coefficients.device, dev))
    try:
        scale = tuple(float(v) for v in band_scale)
    except (TypeError, ValueError):
        raise ValueError('band_scale must be 3 numbers, got %r' % (band_scale,))
    if len(scale) != 3:
        raise ValueError('band_scale must be 3 numbers, got %d' % len(scale))
    lo, hi = _clamp_bounds(clamp)
    flags = (_lib.SHADE_CLAMP if clamp is not None else 0) | (_lib.SHADE_SH_NORMALIZE if normalize else 0)
    # the parameter block: [1 or B, 30]; bands the table does not have stay zeros of the constant row
    slots = [(0, coefficients.to(torch.float32).reshape(-1, 3 * shape[-2])), (3 * _SH_TERMS, _value(background, 3, 'background', dev, batch))]
    return (offsets, scale, lo, hi, flags) + _split_slots(_lib.SHADE_SH_PARAMS, slots)


# ---- Cook-Torrance metallic-roughness lighting (dirt_shade_pbr.hip)

_PBR_KINDS = _lib.SHADE_PBR_KINDS


def pbr_directional_light(direction, color):
    """A light record for `shade_gbuffer_pbr`: light travelling along `direction` (normalised by the shader)."""
    return ('directional', direction, color)


def pbr_point_light(position, color):
    """A light record for `shade_gbuffer_pbr`: a light at `position`, without distance fall-off."""
    return ('point', position, color)


class _ShadeGBufferPBR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, block, colors, material, visibility, meta):
        """colors / material: None (channels of the G-buffer) or float32 [..., 3] / [..., 2] beside it, visibility: None or
        float32 [..., lights]; each read in place under `_stage.rows_in_place`"""
        lib = _lib.load()
        scenes, pixels, cg, offsets, nl, kinds, scalars, lo, hi, flags = meta
        out, block, csrc, msrc, *strides = _forward_operands(gbuffer, block, colors, material)
        vsrc = None
        if visibility is not None:
            vsrc, vstride = _stage.rows_in_place(visibility, nl)
            strides = strides + [vstride]
        if scenes * pixels and vsrc is None:
            _stage.call(lib.dirt_shade_pbr_forward, gbuffer.device, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), block.data_ptr(), out.data_ptr(),
                        scenes, pixels, cg, *strides, *offsets, int(block.shape[0]), nl, kinds, *scalars, lo, hi, flags)
        elif scenes * pixels:
            _stage.call(lib.dirt_shade_pbr_visibility_forward, gbuffer.device, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), vsrc.data_ptr(),
                        block.data_ptr(), out.data_ptr(), scenes, pixels, cg, *strides, *offsets, int(block.shape[0]), nl, kinds, *scalars,
                        lo, hi, flags)
        ctx.save_for_backward(gbuffer, block, csrc, msrc, vsrc)
        ctx.meta, ctx.strides = meta, strides
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, block, csrc, msrc, vsrc = ctx.saved_tensors
        scenes, pixels, cg, offsets, nl, kinds, scalars, lo, hi, flags = ctx.meta
        dev = gbuffer.device
        empty = not scenes * pixels
        (grad_v,) = _stage.dense_grads(grad_out, (nl,), (vsrc is not None and ctx.needs_input_grad[4],), empty)
        grad_g, grad_p, grad_c, grad_m, grad_out = _backward_operands(ctx.needs_input_grad, grad_out, gbuffer, block, empty, csrc, msrc)
        if grad_out is None:
            return grad_g, grad_p, grad_c, grad_m, grad_v, None
        nbytes = lib.dirt_shade_pbr_scratch_bytes(scenes, pixels, nl) if grad_p is not None else 0
        if vsrc is None:
            _stage.call(lib.dirt_shade_pbr_backward, dev, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), block.data_ptr(), grad_out.data_ptr(),
                        _ptr(grad_g), _ptr(grad_c), _ptr(grad_m), _ptr(grad_p), _ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, pixels, cg,
                        *ctx.strides, *offsets, int(block.shape[0]), nl, kinds, *scalars, lo, hi, flags)
        else:
            _stage.call(lib.dirt_shade_pbr_visibility_backward, dev, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), vsrc.data_ptr(), block.data_ptr(),
                        grad_out.data_ptr(), _ptr(grad_g), _ptr(grad_c), _ptr(grad_m), _ptr(grad_v), _ptr(grad_p),
                        _ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, pixels, cg, *ctx.strides, *offsets, int(block.shape[0]), nl, kinds,
                        *scalars, lo, hi, flags)
        return grad_g, grad_p, grad_c, grad_m, grad_v, None


def shade_gbuffer_pbr(gbuffer, lights, *, colors, material, normals, positions, camera_position, mask=None, ambient=(0., 0., 0.),
                      background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04, visibility=None):
    """Lights a G-buffer per pixel with the Cook-Torrance metallic-roughness model in one kernel, differentiably: what
    `lighting.cook_torrance` computes per vertex (GGX distribution, Smith-Schlick visibility, Schlick Fresnel; its docstring
    is the specification), composited and clamped as `shade_gbuffer` does.

    gbuffer, colors (the albedo: channel index or tensor [..., 3]), normals, positions, mask, ambient, background,
        camera_position, clamp: as in `shade_gbuffer`; `positions` and `camera_position` are required.
    material: the first of two consecutive G-buffer channels (roughness, metalness), or a floating-point tensor shaped like the
        G-buffer with 2 channels on its device, differentiable and read in place where its pixels lie a constant stride >= 2
        floats apart: `tex[..., :3]` and `tex[..., 3:5]` of a 5-channel texture look-up serve as colours and material.
    lights: up to 4 records ('directional', direction, color) or ('point', position, color); `pbr_directional_light` and
        `pbr_point_light` build them.  Vectors and colours: 3 numbers or a tensor [3], or [B, 3] with a [B, H, W, Cg] G-buffer;
        tensors are differentiable.  Directions are normalised by the shader; point lights have no distance fall-off.
    min_roughness (in (0, 1]: the roughness is clamped to [min_roughness, 1]) and dielectric_f0 (in [0, 1]: the Fresnel
        reflectance of a non-metal at normal incidence): python numbers, not differentiable.
    visibility: None, or a floating-point tensor shaped like the G-buffer with len(lights) channels on its device -- the output
        of `shadow_visibility`: light i's term is multiplied by visibility[..., i], as it is (no clamp; the ambient term is not
        shadowed; all ones give the bits of the call without it).  Differentiable, and read in place where its pixels lie a
        constant stride >= len(lights) floats apart (`shadow_visibility`'s output, a slice `t[..., 1:1 + L]`).  There is no
        channel-index form: the look-up's output is a tensor of its own, and the G-buffer's gradient tile has no slot for it.

    Returns [..., 3]:  clamp((ambient * c + sum of the lights' terms) * m + background * (1 - m), lo, hi).
    Gradients are those of torch's autograd for that composition, including at the kinks (max(x, 0) and the clamps pass the
    gradient at their edges, the norm of a zero vector has gradient 0).  A zero normal makes the distribution term a2 / 0 and
    the pixel inf * 0 = NaN whatever its mask, as in `lighting.cook_torrance`: give the uncovered pixels of a deferred renderer
    a unit normal (examples/fit_material_fused.py::background_attributes)."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'shade_gbuffer_pbr')
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.shade_gbuffer_pbr')
    lights = list(lights)
    offsets, kinds, scalars, lo, hi, flags, const, tensors = _check_pbr_arguments(gbuffer, lights, colors, material, normals, positions, mask,
                                                                                   ambient, camera_position, background, clamp, min_roughness,
                                                                                   dielectric_f0)
    _check_pbr_visibility(gbuffer, len(lights), visibility)
    block = _splice_block(gbuffer.device, const, tensors)
    meta = (scenes, pixels, cg, tuple(offsets), len(lights), kinds, scalars, lo, hi, flags)
    return _ShadeGBufferPBR.apply(g, block, _as_input(colors), _as_input(material), _as_input(visibility), meta)


def _check_pbr_visibility(gbuffer, n_lights, visibility):
    """What `shade_gbuffer_pbr` refuses of its `visibility` with a ValueError, on shapes and devices alone (after
    `_check_pbr_arguments`; None passes)."""
    if visibility is None:
        return
    if not isinstance(visibility, torch.Tensor):
        raise ValueError('visibility must be a tensor (there is no channel-index form), got %r' % (visibility,))
    if n_lights == 0:
        raise ValueError('visibility needs at least one light, got none')
    want = list(gbuffer.shape[:-1]) + [n_lights]
    if list(visibility.shape) != want:
        raise ValueError("visibility must have shape %s (the G-buffer's %s with one channel per light), got %s"
                         % (want, list(gbuffer.shape), list(visibility.shape)))
    if not visibility.dtype.is_floating_point:
        raise ValueError('visibility must be floating-point, got %s' % visibility.dtype)
    if visibility.device != gbuffer.device:
        raise ValueError('visibility is on %s, the G-buffer on %s' % (visibility.device, gbuffer.device))


def _check_pbr_arguments(gbuffer, lights, colors, material, normals, positions, mask, ambient, camera_position, background, clamp,
                         min_roughness, dielectric_f0):
    """Everything `shade_gbuffer_pbr` refuses with a ValueError, on shapes and devices alone (no device work): -> (channel
    offsets (colors, material, normals, positions, mask), light kinds, (min_roughness, dielectric_f0), lo, hi, flags, the
    block's constant row, [(first slot, tensor [1 or B, width])])."""
    dev, batch = _check_gbuffer(gbuffer, 'shade_gbuffer_pbr')
    offsets = _channel_offsets(gbuffer, (('colors', colors, 3, True), ('material', material, 2, True), ('normals', normals, 3, True),
                                         ('positions', positions, 3, True), ('mask', mask, 1, False)))
    if len(lights) > _lib.SHADE_PBR_MAX_LIGHTS:
        raise ValueError('shade_gbuffer_pbr takes at most %d lights, got %d' % (_lib.SHADE_PBR_MAX_LIGHTS, len(lights)))
    scalars = _material_scalars(min_roughness, dielectric_f0)
    if camera_position is None:
        raise ValueError('shade_gbuffer_pbr needs camera_position')
    lo, hi = _clamp_bounds(clamp)
    flags = _lib.SHADE_CLAMP if clamp is not None else 0
    # the parameter block: [1 or B, 9 + 8 lights] in the layout of `_light_block`
    slots = _param_head(ambient, background, camera_position, dev, batch)
    kinds = 0
    for l, rec in enumerate(lights):
        if not isinstance(rec, (tuple, list)) or not rec or rec[0] not in _PBR_KINDS:
            raise ValueError('light %d: expected a record starting with one of %s, got %r' % (l, sorted(_PBR_KINDS), rec))
        if len(rec) != 3:
            raise ValueError('light %d: a %s record has 3 fields, got %d' % (l, rec[0], len(rec)))
        base = _lib.SHADE_PARAM_HEAD + _lib.SHADE_PARAM_LIGHT * l
        slots.append((base, _value(rec[1], 3, 'light %d %s' % (l, 'position' if rec[0] == 'point' else 'direction'), dev, batch)))
        slots.append((base + 3, _value(rec[2], 3, 'light %d color' % l, dev, batch)))
        kinds |= _PBR_KINDS[rec[0]] << l
    return (offsets, kinds, scalars, lo, hi, flags) + _split_slots(_lib.SHADE_PARAM_HEAD + _lib.SHADE_PARAM_LIGHT * len(lights), slots)


def _material_scalars(min_roughness, dielectric_f0):
    """The two python numbers of the material model, refused outside their ranges -> (min_roughness, dielectric_f0) as floats."""
    scalars = []
    for name, x, text, ok in (('min_roughness', min_roughness, '> 0 and <= 1', lambda v: 0. < v <= 1.),
                              ('dielectric_f0', dielectric_f0, 'in [0, 1]', lambda v: 0. <= v <= 1.)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or not ok(float(x)):
            raise ValueError('%s must be a number %s, got %r' % (name, text, x))
        scalars.append(float(x))
    return tuple(scalars)


# ---- split-sum image-based lighting (dirt_shade_ibl.hip)

class _ShadeGBufferIBL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, block, colors, material, packed, irradiance, brdf, meta):
        """colors / material: None (channels of the G-buffer) or float32 [..., 3] / [..., 2] beside it, read in place under
        `_stage.rows_in_place`; packed [6, floats], irradiance [6, M, M, 3], brdf [S, S, 2]: float32"""
        lib = _lib.load()
        scenes, rows, cols, cg, offsets, sizes, scalars, lo, hi, flags = meta
        out, block, csrc, msrc, *strides = _forward_operands(gbuffer, block, colors, material)
        packed, irradiance, brdf = packed.contiguous(), irradiance.contiguous(), brdf.contiguous()
        if scenes * rows * cols:
            _stage.call(lib.dirt_shade_ibl_forward, gbuffer.device, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), block.data_ptr(),
                        packed.data_ptr(), irradiance.data_ptr(), brdf.data_ptr(), out.data_ptr(), scenes, rows, cols, cg, *strides,
                        *offsets, int(block.shape[0]), *sizes, *scalars, lo, hi, flags)
        ctx.save_for_backward(gbuffer, block, csrc, msrc, packed, irradiance, brdf)
        ctx.meta, ctx.strides = meta, strides
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, block, csrc, msrc, packed, irradiance, brdf = ctx.saved_tensors
        scenes, rows, cols, cg, offsets, sizes, scalars, lo, hi, flags = ctx.meta
        dev = gbuffer.device
        empty = not scenes * rows * cols
        grad_g, grad_p, grad_c, grad_m, grad_out = _backward_operands(ctx.needs_input_grad, grad_out, gbuffer, block, empty, csrc, msrc)
        grad_s, grad_i = _stage.grad_outputs((packed, irradiance), ctx.needs_input_grad[4:6], empty)   # the cubes': cleared by the call
        if empty:
            return grad_g, grad_p, grad_c, grad_m, grad_s, grad_i, None, None
        nbytes = lib.dirt_shade_ibl_scratch_bytes(scenes, rows, cols) if grad_p is not None or grad_s is not None or grad_i is not None else 0
        _stage.call(lib.dirt_shade_ibl_backward, dev, gbuffer.data_ptr(), _ptr(csrc), _ptr(msrc), block.data_ptr(), packed.data_ptr(),
                    irradiance.data_ptr(), brdf.data_ptr(), grad_out.data_ptr(), _ptr(grad_g), _ptr(grad_c), _ptr(grad_m), _ptr(grad_p),
                    _ptr(grad_s), _ptr(grad_i), _ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, rows, cols, cg, *ctx.strides, *offsets,
                    int(block.shape[0]), *sizes, *scalars, lo, hi, flags)
        return grad_g, grad_p, grad_c, grad_m, grad_s, grad_i, None, None


def shade_gbuffer_ibl(gbuffer, specular, irradiance, brdf, *, colors, material, normals, positions, camera_position, mask=None,
                      intensity=(1., 1., 1.), background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04):
    """Lights a G-buffer per pixel with the material of `shade_gbuffer_pbr` under an environment, by the split sum, in one
    kernel, differentiably: what `lighting.image_based_lighting` computes per vertex (its docstring is the specification),
    composited and clamped as `shade_gbuffer` does.

    specular: the 3-channel `CubePyramid` of `texture.prefilter_cube(environment)` with its default roughness ramp k / (L - 1),
        looked up at the mirrored view vector at lod = roughness (L - 1).
    irradiance: [6, M, M, 3], `texture.convolve_cube(environment_mip, kind='lambert')`, looked up at the normal as it stands in
        the G-buffer: an all-zero normal -- a background pixel -- gets no irradiance.
    brdf: [S, S, 2] with 2 <= S <= 128 on the G-buffer's device, `lighting.environment_brdf(S).to(device)`: built once per fit.
    gbuffer, colors, material, normals, positions, mask, background, camera_position, clamp, min_roughness, dielectric_f0: as
        in `shade_gbuffer_pbr`.  intensity: the environment's scale per channel; like background and camera_position 3 numbers
        or a tensor [3], or [B, 3] with a [B, H, W, Cg] G-buffer, differentiable.
    One cube pair serves every scene of a batch.

    Returns [..., 3]:  clamp(L * m + background * (1 - m), lo, hi)  with
    L = intensity ((1 - S)(1 - mu) c E + S spec), S = F0 A + B.  Gradients are those of torch's autograd for that composition
    (the kinks as in `shade_gbuffer_pbr`; an invalid direction adds nothing) and go to the G-buffer, the colour and material
    tensors, the three parameters, `specular.packed` (and through it the environment) and `irradiance`; none goes to `brdf`.
    The cubes' gradients are summed with float atomics where a 16 x 16 tile of pixels straddles faces: they are not the same
    bits on every run, everything else is.

    Direct lights are added by the caller: `shade_gbuffer_pbr(..., clamp=None) + shade_gbuffer_ibl(..., clamp=None)`, then
    one clamp.  The environment behind the mesh, in place of the flat `background`, likewise:
    `(shade_gbuffer_ibl(..., background=(0., 0., 0.), clamp=None) + environment_background(specular, clip_to_world, (H, W),
    mask=gbuffer[..., mask], filter='trilinear')).clamp(0., 1.)` -- `specular`'s level 0 is the environment itself."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'shade_gbuffer_ibl')
    offsets, sizes, scalars, lo, hi, flags, const, tensors = _check_ibl_arguments(gbuffer, specular, irradiance, brdf, colors, material, normals,
                                                                                   positions, mask, intensity, camera_position, background, clamp,
                                                                                   min_roughness, dielectric_f0)
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.shade_gbuffer_ibl')
    block = _splice_block(gbuffer.device, const, tensors)
    # a scene's pixel grid: the image's rows and columns, one row for a flat list
    rows, cols = (int(gbuffer.shape[-3]), int(gbuffer.shape[-2])) if gbuffer.dim() >= 3 else (1, pixels)
    meta = (scenes, rows, cols, cg, tuple(offsets), sizes, scalars, lo, hi, flags)
    return _ShadeGBufferIBL.apply(g, block, _as_input(colors), _as_input(material), _as_input(specular.packed), _as_input(irradiance),
                                  _as_input(brdf), meta)


def _check_ibl_arguments(gbuffer, specular, irradiance, brdf, colors, material, normals, positions, mask, intensity, camera_position,
                         background, clamp, min_roughness, dielectric_f0):
    """Everything `shade_gbuffer_ibl` refuses with a ValueError, on types, shapes and devices alone (no device work): -> (channel
    offsets (colors, material, normals, positions, mask), (pyramid size, levels, irradiance size, table size), (min_roughness,
    dielectric_f0), lo, hi, flags, the block's constant row, [(first slot, tensor [1 or B, width])])."""
    from .texture import CubePyramid, _cube_level
    who = 'shade_gbuffer_ibl'
    dev, batch = _check_gbuffer(gbuffer, who)
    if not isinstance(specular, CubePyramid):
        raise ValueError('%s expects specular to be the CubePyramid of prefilter_cube, got %s' % (who, type(specular).__name__))
    if specular.roughness is None:
        raise ValueError('%s: specular is a box-filtered pyramid (roughness None): the look-up at lod = roughness (L - 1) needs the '
                         'levels prefilter_cube convolves' % who)
    ramp = tuple(k / (specular.levels - 1) for k in range(specular.levels)) if specular.levels > 1 else (0.0,)
    if specular.roughness != ramp:
        raise ValueError('%s: specular was filtered at the roughnesses %r, the look-up at lod = roughness (L - 1) needs the default '
                         'ramp k / (L - 1) of prefilter_cube' % (who, specular.roughness))
    if specular.channels != 3:
        raise ValueError('%s: specular has %d channels, an environment has 3' % (who, specular.channels))
    top, top_size = _cube_level(specular.size, 3, specular.levels - 1)
    if not isinstance(specular.packed, torch.Tensor) or tuple(specular.packed.shape) != (6, top + top_size * top_size * 3):
        raise ValueError('%s: specular.packed must be [6, %d], the %d levels of a %d x %d x 3 face, got %s'
                         % (who, top + top_size * top_size * 3, specular.levels, specular.size, specular.size,
                            tuple(getattr(specular.packed, 'shape', ()))))
    if not isinstance(irradiance, torch.Tensor) or irradiance.dim() != 4 or irradiance.shape[0] != 6 or irradiance.shape[1] != irradiance.shape[2] \
            or irradiance.shape[3] != 3 or 0 in irradiance.shape or not irradiance.is_floating_point():
        raise ValueError('%s expects irradiance to be a floating-point tensor [6, size, size, 3], got %s'
                         % (who, tuple(getattr(irradiance, 'shape', ()))))
    if not isinstance(brdf, torch.Tensor) or brdf.dim() != 3 or brdf.shape[0] != brdf.shape[1] or brdf.shape[2] != 2 \
            or not 2 <= brdf.shape[0] <= _lib.SHADE_IBL_MAX_TABLE or not brdf.is_floating_point():
        raise ValueError('%s expects brdf to be a floating-point tensor [S, S, 2] with 2 <= S <= %d (lighting.environment_brdf), got %s'
                         % (who, _lib.SHADE_IBL_MAX_TABLE, tuple(getattr(brdf, 'shape', ()))))
    for name, t in (('specular', specular.packed), ('irradiance', irradiance), ('brdf', brdf)):
        if t.device != dev:
            raise ValueError('%s is on %s, the G-buffer on %s' % (name, t.device, dev))
    offsets = _channel_offsets(gbuffer, (('colors', colors, 3, True), ('material', material, 2, True), ('normals', normals, 3, True),
                                         ('positions', positions, 3, True), ('mask', mask, 1, False)))
    scalars = _material_scalars(min_roughness, dielectric_f0)
    if camera_position is None:
        raise ValueError('%s needs camera_position' % who)
    lo, hi = _clamp_bounds(clamp)
    flags = _lib.SHADE_CLAMP if clamp is not None else 0
    # the parameter block: [1 or B, 9] in the layout of `_param_head`, the intensity in the ambient slot
    slots = [(0, _value(intensity, 3, 'intensity', dev, batch))] + _param_head((0., 0., 0.), background, camera_position, dev, batch)[1:]
    sizes = (specular.size, specular.levels, int(irradiance.shape[1]), int(brdf.shape[0]))
    return (offsets, sizes, scalars, lo, hi, flags) + _split_slots(_lib.SHADE_PARAM_HEAD, slots)


# ---- tangent-space normal mapping (dirt_normal_map.hip)

class _PerturbNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, normal_map, meta):
        """normal_map: float32 [..., 3] beside the G-buffer, read in place under `_stage.rows_in_place`"""
        lib = _lib.load()
        scenes, pixels, cg, offsets, strength, flags = meta
        out = torch.empty_like(gbuffer)
        src, stride = _stage.rows_in_place(normal_map, 3)
        if scenes * pixels:
            _stage.call(lib.dirt_normal_map_forward, gbuffer.device, gbuffer.data_ptr(), src.data_ptr(), out.data_ptr(), scenes, pixels, cg, stride,
                        *offsets, strength, flags)
        ctx.save_for_backward(gbuffer, src)
        ctx.meta, ctx.map_stride = meta, stride
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, src = ctx.saved_tensors
        scenes, pixels, cg, offsets, strength, flags = ctx.meta
        grad_g, = _stage.grad_outputs((gbuffer,), ctx.needs_input_grad[:1], not scenes * pixels)
        grad_m, = _stage.dense_grads(grad_out, (3,), ctx.needs_input_grad[1:2], not scenes * pixels)
        if not scenes * pixels:
            return grad_g, grad_m, None
        grad_out = grad_out.to(torch.float32).contiguous()
        _stage.call(lib.dirt_normal_map_backward, gbuffer.device, gbuffer.data_ptr(), src.data_ptr(), grad_out.data_ptr(), _ptr(grad_g),
                    _ptr(grad_m), scenes, pixels, cg, ctx.map_stride, *offsets, strength, flags)
        return grad_g, grad_m, None


def perturb_normals(gbuffer, normal_map, *, normals, tangents, strength=1.0, encoded=True):
    """Tangent-space normal mapping of a G-buffer in one kernel, differentiably: what `lighting.perturb_normals` computes
    per element, written back into the G-buffer, so that no `torch.cat` stands between a texture look-up and a shader.

    gbuffer: float32 [H, W, Cg], [B, H, W, Cg] or a flat [N, Cg] on the GPU, as the shaders take it.
    normals, tangents: the first channel of the interpolated normal (3 channels) and of the interpolated tangent frame of
        `geometry.vertex_tangents` (4 channels: tangent and handedness) inside a pixel; no overlap.
    normal_map: a floating-point tensor shaped like the G-buffer with 3 channels on its device, differentiable.  One whose
        pixels lie a constant stride >= 3 floats apart -- `tex[..., 5:8]` of an 8-channel texture look-up -- is read in place.
    strength: a python number multiplying the decoded x and y (0: the normals are only renormalised); not differentiable.
    encoded: the map holds (d + 1) / 2, as an image file does, and is decoded as 2 m - 1; otherwise it holds d itself.

    Returns a new G-buffer of the same shape: the normal channels hold the shading normal (unit), every other channel the
    input's bits; `shade_gbuffer`, `shade_gbuffer_sh` and `shade_gbuffer_pbr` take it with the same channel indices.
    A pixel with a zero normal (a background), with no tangent orthogonal to its normal or with a zero decoded vector keeps
    its normal and passes the incoming gradient to it alone.  Gradients are those of torch's autograd for
    `lighting.perturb_normals`: to the normal, tangent and handedness channels of the G-buffer (the other channels pass
    theirs through) and to the normal map (dense [..., 3])."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'perturb_normals')
    offsets, strength, flags = _check_normal_map_arguments(gbuffer, normal_map, normals, tangents, strength, encoded)
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.perturb_normals')
    return _PerturbNormals.apply(g, normal_map.to(torch.float32), (scenes, pixels, cg, tuple(offsets), strength, flags))


def _check_normal_map_arguments(gbuffer, normal_map, normals, tangents, strength, encoded):
    """Everything `perturb_normals` refuses with a ValueError, on shapes and devices alone (no device work): -> (channel offsets
    (normals, tangents), strength, flags)"""
    _check_gbuffer(gbuffer, 'perturb_normals')
    offsets = _channel_offsets(gbuffer, (('normals', normals, 3, True), ('tangents', tangents, 4, True)))
    want = tuple(gbuffer.shape[:-1]) + (3,)
    if not isinstance(normal_map, torch.Tensor) or not normal_map.dtype.is_floating_point:
        raise ValueError('normal_map must be a floating-point tensor, got %s' % (getattr(normal_map, 'dtype', type(normal_map).__name__),))
    if tuple(normal_map.shape) != want:
        raise ValueError('normal_map must have shape %s (the G-buffer\'s %s with 3 channels), got %s'
                         % (list(want), list(gbuffer.shape), list(normal_map.shape)))
    if normal_map.device != gbuffer.device:
        raise ValueError('normal_map is on %s, the G-buffer on %s' % (normal_map.device, gbuffer.device))
    if isinstance(strength, bool) or not isinstance(strength, numbers.Real):
        raise ValueError('strength must be a number, got %r' % (strength,))
    return offsets, float(strength), _lib.NORMAL_MAP_ENCODED if encoded else 0


# ---- shadow maps (dirt_shadow.hip)

class _ShadowVisibility(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gbuffer, maps, matrices, meta):
        """maps [1 or B, L, Hs, Ws], matrices [1 or B, L, 4, 4]: float32"""
        lib = _lib.load()
        scenes, rows, cols, cg, offsets, lights, hs, ws, scalars = meta
        maps, matrices = maps.contiguous(), matrices.contiguous()
        out = torch.empty(tuple(gbuffer.shape[:-1]) + (lights,), dtype=torch.float32, device=gbuffer.device)
        if scenes * rows * cols:
            _stage.call(lib.dirt_shadow_forward, gbuffer.device, gbuffer.data_ptr(), maps.data_ptr(), matrices.data_ptr(), out.data_ptr(),
                        scenes, rows * cols, cg, *offsets, lights, hs, ws, int(maps.shape[0]), int(matrices.shape[0]), *scalars)
        ctx.save_for_backward(gbuffer, maps, matrices)
        ctx.meta = meta
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        gbuffer, maps, matrices = ctx.saved_tensors
        scenes, rows, cols, cg, offsets, lights, hs, ws, scalars = ctx.meta
        dev = gbuffer.device
        empty = not scenes * rows * cols
        grad_g, grad_s, grad_m = _stage.grad_outputs((gbuffer, maps, matrices), ctx.needs_input_grad[:3], empty)
        if empty:
            return grad_g, grad_s, grad_m, None
        grad_out = grad_out.to(torch.float32).contiguous()
        nbytes = lib.dirt_shadow_scratch_bytes(scenes, rows, cols, lights) if grad_m is not None else 0
        _stage.call(lib.dirt_shadow_backward, dev, gbuffer.data_ptr(), maps.data_ptr(), matrices.data_ptr(), grad_out.data_ptr(), _ptr(grad_g),
                    _ptr(grad_s), _ptr(grad_m), _ptr(_stage.scratch(dev, nbytes)), nbytes, scenes, rows, cols, cg, *offsets, lights, hs, ws,
                    int(maps.shape[0]), int(matrices.shape[0]), *scalars)
        return grad_g, grad_s, grad_m, None


def shadow_visibility(gbuffer, shadow_maps, light_matrices, *, positions, normals=None, mask=None, kernel=3, bias=0.0, softness,
                      normal_offset=0.0):
    """The share of each light that reaches each pixel of a G-buffer, looked up in the lights' shadow maps in one kernel,
    differentiably: what `lighting.shadow_visibility` computes per point (its docstring is the specification).

    gbuffer: float32 [H, W, Cg], [B, H, W, Cg] or a flat [N, Cg] on the GPU; a contiguous one is read in place.
    positions, normals, mask: the first channel of each attribute inside a pixel (3, 3 and 1 channels; any order, no
        overlap).  `positions` holds world-space positions; `normals` is needed only with normal_offset != 0; mask=None:
        every pixel is covered.
    shadow_maps: float32 [L, Hs, Ws] with 1 <= L <= 4 (the light count of `shade_gbuffer_pbr`), the clip-space z of the
        nearest surface as each light sees it: `render_shadow_map` draws one.
    light_matrices: [L, 4, 4], world -> each light's clip space, right-multiplying row vectors as everything in `matrices`
        and `vertex_stage`'s view_projection: the matrix its map was drawn with.
    With a [B, H, W, Cg] G-buffer either may have a leading B ([B, L, Hs, Ws], [B, L, 4, 4]): an operand shared by the scenes
        has no leading B, one with a leading B has one value per scene.
    kernel: the side of the percentage-closer filter, 1, 3 or 5.  bias: added to the map's depth before the comparison (in
        clip z).  softness > 0: the width in clip z over which the comparison goes from shadow to light (one whose float32
        reciprocal is not finite, below 2.94e-39, is refused: the kernel multiplies by it).  normal_offset: the
        distance in world units the point is moved along its unit normal before it is projected.  Python numbers, no gradient.

    Returns [..., L]:  1 - m (1 - v)  with v in [0, 1] the filtered comparison: 1 = lit, 0 = in shadow; an uncovered pixel, one
    behind the light and one whose filter window lies off the map are lit.  Gradients are those of torch's autograd for
    `lighting.shadow_visibility` and go to the position channels of the G-buffer, its normal channels when used and its mask
    channel (every other channel gets an exact zero), to `shadow_maps` and to `light_matrices`.  The maps' gradient is summed
    with float atomics: it is not the same bits on every run, everything else is.

    `shade_gbuffer_pbr(gbuffer, lights, ..., visibility=vis)` takes the result as it is and shadows its lights in the one call.
    The other shaders have no such operand: there a shadowed light is a call with that light alone (`ambient=(0, 0, 0),
    background=(0, 0, 0), clamp=None`) times `vis[..., i:i + 1]`, summed over the lights, plus the ambient or image-based term
    (`shade_gbuffer_ibl(..., clamp=None)`) and the background, under one clamp."""
    g, scenes, pixels, cg = _gbuffer_sizes(gbuffer, 'shadow_visibility')
    offsets, lights, hs, ws, scalars = _check_shadow_arguments(gbuffer, shadow_maps, light_matrices, positions, normals, mask, kernel, bias,
                                                               softness, normal_offset)
    _stage.require_gpu(gbuffer, 'dirt_amd.shading.shadow_visibility')
    rows, cols = (int(gbuffer.shape[-3]), int(gbuffer.shape[-2])) if gbuffer.dim() >= 3 else (1, pixels)
    maps, matrices = shadow_maps.to(torch.float32), light_matrices.to(torch.float32)
    maps = maps if maps.dim() == 4 else maps[None]
    matrices = matrices if matrices.dim() == 4 else matrices[None]
    return _ShadowVisibility.apply(g, maps, matrices, (scenes, rows, cols, cg, tuple(offsets), lights, hs, ws, scalars))


def _check_shadow_arguments(gbuffer, shadow_maps, light_matrices, positions, normals, mask, kernel, bias, softness, normal_offset):
    """Everything `shadow_visibility` refuses with a ValueError, on types, shapes and devices alone (no device work): -> (channel
    offsets (positions, normals, mask), lights, map height, map width, (kernel, bias, softness, normal_offset))."""
    from .lighting import _shadow_scalars
    who = 'shadow_visibility'
    dev, batch = _check_gbuffer(gbuffer, who)
    ranks = (3, 4) if batch is not None else (3,)
    forms = '[L, Hs, Ws] or [B, L, Hs, Ws]' if batch is not None else '[L, Hs, Ws]'
    if not isinstance(shadow_maps, torch.Tensor) or not shadow_maps.is_floating_point() or shadow_maps.dim() not in ranks \
            or not 1 <= shadow_maps.shape[-3] <= _lib.SHADOW_MAX_LIGHTS or 0 in shadow_maps.shape[-2:]:
        raise ValueError('%s expects shadow_maps to be a floating-point tensor %s with 1 <= L <= %d and no empty map, got %s'
                         % (who, forms, _lib.SHADOW_MAX_LIGHTS, tuple(getattr(shadow_maps, 'shape', ()))))
    lights, hs, ws = (int(s) for s in shadow_maps.shape[-3:])
    forms = '[%d, 4, 4] or [B, %d, 4, 4]' % (lights, lights) if batch is not None else '[%d, 4, 4]' % lights
    if not isinstance(light_matrices, torch.Tensor) or not light_matrices.is_floating_point() or light_matrices.dim() not in ranks \
            or tuple(light_matrices.shape[-3:]) != (lights, 4, 4):
        raise ValueError('%s expects light_matrices to be a floating-point tensor %s, a matrix per map, got %s'
                         % (who, forms, tuple(getattr(light_matrices, 'shape', ()))))
    for name, t in (('shadow_maps', shadow_maps), ('light_matrices', light_matrices)):
        if t.dim() == 4 and int(t.shape[0]) != batch:
            raise ValueError('%s: %d scenes of gbuffer, %d of %s' % (who, batch, int(t.shape[0]), name))
        if t.device != dev:
            raise ValueError('%s is on %s, the G-buffer on %s' % (name, t.device, dev))
    offsets = _channel_offsets(gbuffer, (('positions', positions, 3, True), ('normals', normals, 3, False), ('mask', mask, 1, False)))
    scalars = _shadow_scalars(kernel, bias, softness, normal_offset)
    if scalars[3] != 0. and normals is None:
        raise ValueError('%s: normal_offset=%r needs normals' % (who, normal_offset))
    return offsets, lights, hs, ws, scalars


def _shadow_map_operands(vertices, light_matrix, size, far):
    """What `render_shadow_map` hands to the rasteriser, for one scene or a batch: -> (background [..., Hs, Ws, 1] = far, clip
    vertices [..., V, 4] = [v, 1] @ M, vertex colours [..., V, 1] = clip z)."""
    from .lighting import _image_size
    hs, ws = _image_size(size)
    if isinstance(far, bool) or not isinstance(far, numbers.Real) or not math.isfinite(far):
        raise ValueError('far must be a finite number, the clip z of the light\'s far plane, got %r' % (far,))
    v = vertices.to(torch.float32)
    clip = torch.matmul(torch.cat([v, torch.ones_like(v[..., :1])], dim=-1), light_matrix.to(torch.float32))
    background = torch.full(tuple(v.shape[:-2]) + (int(hs), int(ws), 1), float(far), dtype=torch.float32, device=v.device)
    return background, clip, clip[..., 2:3]


def render_shadow_map(vertices, faces, light_matrix, size, far):
    """The shadow map of one light: vertices [V, 3] (world space), faces [F, 3], light_matrix [4, 4] (world -> the light's clip
    space, row vectors: `matrices.compose(view, matrices.orthographic_projection(...))` for a directional light, with
    `perspective_projection` for a spot light), size (an int or (Hs, Ws)) -> float32 [Hs, Ws], the clip-space z of the nearest
    surface per texel and `far` where there is none.  One 1-channel `rasterise` with the clip z as the vertex colour (clip z is
    linear in the world position, so the perspective-correct interpolation is exact for either projection); differentiable
    to the vertices and the matrix through the rasteriser's gradient.

    far: required, the clip z of the light's far plane (1 for an orthographic light, the far distance for a perspective one).
    The rasteriser's gradient at a silhouette scales with the step between the surface and the background, so a huge sentinel
    in place of the far plane would blow it up.

    `shadow_visibility` takes `torch.stack` of the lights' maps with the stack of their matrices."""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError('render_shadow_map expects vertices [V, 3], got %s' % (tuple(getattr(vertices, 'shape', ())),))
    if not isinstance(light_matrix, torch.Tensor) or tuple(light_matrix.shape) != (4, 4):
        raise ValueError('render_shadow_map expects light_matrix [4, 4], got %s' % (tuple(getattr(light_matrix, 'shape', ())),))
    from .rasterise_ops import rasterise
    background, clip, depth = _shadow_map_operands(vertices, light_matrix, size, far)
    return rasterise(background, clip, depth, faces)[..., 0]


def render_shadow_map_batch(vertices, faces, light_matrices, size, far):
    """`render_shadow_map` for a batch: vertices [B, V, 3], faces [F, 3] (one topology for the batch) or [B, F, 3],
    light_matrices [B, 4, 4] or [4, 4] (one light for every scene) -> [B, Hs, Ws], by one `rasterise_batch`."""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 3 or vertices.shape[2] != 3:
        raise ValueError('render_shadow_map_batch expects vertices [B, V, 3], got %s' % (tuple(getattr(vertices, 'shape', ())),))
    if not isinstance(light_matrices, torch.Tensor) or tuple(light_matrices.shape) not in ((4, 4), (int(vertices.shape[0]), 4, 4)):
        raise ValueError('render_shadow_map_batch expects light_matrices [4, 4] or [%d, 4, 4], got %s'
                         % (int(vertices.shape[0]), tuple(getattr(light_matrices, 'shape', ())),))
    from .rasterise_ops import rasterise_batch
    background, clip, depth = _shadow_map_operands(vertices, light_matrices, size, far)
    return rasterise_batch(background, clip, depth, faces)[..., 0]


# ---- the environment behind the mesh (dirt_background.hip)

class _EnvironmentBackground(torch.autograd.Function):
    @staticmethod
    def forward(ctx, environment, matrices, intensity, mask, meta):
        """environment: a cube [6, N, N, 3] or (`packed`) a pyramid [6, floats]; matrices [1 or B, 4, 4], intensity [1 or B, 3]:
        float32; mask: None or [H, W] / [B, H, W], read in place where its values lie a constant stride apart"""
        from .texture import _call_entry, _mip_geometry, _scalars_in_place
        lib = _lib.load()
        scenes, batched, rows, cols, n, levels, packed, code, flags, lod, lod_bias, max_level = meta
        dev = environment.device
        pyr, matrices, intensity = environment.contiguous(), matrices.contiguous(), intensity.contiguous()
        if not packed and code == _lib.BACKGROUND_FILTERS['trilinear']:   # the box pyramid of the cube, built per call
            levels, floats, _ = _mip_geometry(n, n, 3, max_level)
            pyr = torch.empty((6, floats), dtype=torch.float32, device=dev)
            _call_entry('mip_build', 6, dev, (environment.data_ptr(), pyr.data_ptr()), n, n, 3, levels)
        msrc, mstride = _scalars_in_place(mask) if mask is not None else (None, 0)
        out = torch.empty(((scenes,) if batched else ()) + (rows, cols, 3), dtype=torch.float32, device=dev)
        sizes = (scenes, rows, cols, n, levels, int(matrices.shape[0]), int(intensity.shape[0]), 1 if mask is None or mask.dim() == 2 else scenes,
                 mstride, code, lod, lod_bias, flags)
        if scenes * rows * cols:
            _stage.call(lib.dirt_background_forward, dev, pyr.data_ptr(), matrices.data_ptr(), intensity.data_ptr(), _ptr(msrc), out.data_ptr(), *sizes)
        ctx.save_for_backward(pyr, matrices, intensity, msrc)
        ctx.meta, ctx.sizes, ctx.mask_shape = meta, sizes, None if mask is None else tuple(mask.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from .texture import _call_entry
        lib = _lib.load()
        pyr, matrices, intensity, msrc = ctx.saved_tensors
        scenes, batched, rows, cols, n, levels, packed, code, flags, lod, lod_bias, max_level = ctx.meta
        dev = pyr.device
        empty = not scenes * rows * cols
        want_env, want_m, want_i, want_mask = ctx.needs_input_grad[:4]
        grad_pyr, grad_m, grad_i = _stage.grad_outputs((pyr, matrices, intensity), (want_env, want_m, want_i), empty)   # the pyramid's: cleared by the call
        grad_mask, = _stage.dense_grads(grad_out.reshape(scenes, rows, cols, 3), (1,), (want_mask and msrc is not None,), empty)   # [scenes, H, W, 1]
        if not empty:
            grad_out = grad_out.to(torch.float32).contiguous()
            nbytes = lib.dirt_background_scratch_bytes(scenes, rows, cols) if want_env or want_m or want_i else 0
            _stage.call(lib.dirt_background_backward, dev, pyr.data_ptr(), matrices.data_ptr(), intensity.data_ptr(), _ptr(msrc), grad_out.data_ptr(),
                        _ptr(grad_pyr), _ptr(grad_m), _ptr(grad_i), _ptr(grad_mask), _ptr(_stage.scratch(dev, nbytes)), nbytes, *ctx.sizes)
        grad_env = grad_pyr
        if grad_pyr is not None and not packed:   # the operand was a cube: level 0 itself, or the pyramid's collapse
            if grad_pyr.numel() == 6 * n * n * 3:
                grad_env = grad_pyr.view(6, n, n, 3)
            else:
                grad_env = torch.empty((6, n, n, 3), dtype=torch.float32, device=dev)
                _call_entry('mip_collapse', 6, dev, (grad_pyr.data_ptr(), grad_env.data_ptr()), n, n, 3, int(ctx.sizes[4]))
        if grad_mask is not None:   # a mask shared by the scenes: summed over them, in scene order
            grad_mask = grad_mask[..., 0].sum(0) if len(ctx.mask_shape) == 2 else grad_mask
            grad_mask = grad_mask.reshape(ctx.mask_shape)
        return grad_env, grad_m, grad_i, grad_mask, None


def environment_background(environment, clip_to_world, size, *, mask=None, intensity=(1., 1., 1.), filter='bilinear', lod=None, lod_bias=0.0,
                           max_level=None):
    """The environment seen behind the mesh, in one kernel, differentiably: what `lighting.environment_background` computes
    per pixel (its docstring is the specification) -- the cube looked up along the ray through each pixel's centre, with no
    ray image, no pixel grid and no look-up where the mesh covers the pixel.

    environment: a float32 cube [6, N, N, 3] on the GPU, as `sample_texture_cube` takes it (with filter='trilinear' its box
        pyramid is built per call), or a 3-channel `CubePyramid` (`cube_pyramid`, or the `prefilter_cube` pyramid that
        `shade_gbuffer_ibl` holds: its level 0 is the environment itself, so one pyramid serves both calls) with
        filter='trilinear'; the gradient then goes to `environment.packed`.  One environment serves every scene.
    clip_to_world: [4, 4] or [B, 4, 4], what `projection.unproject_pixels_to_rays` takes (row vectors, typically
        inverse(view @ projection)); differentiable.
    size: an int or (height, width), as `render_shadow_map` takes it.
    mask: None (every pixel is background) or a float tensor [H, W] / [B, H, W], 1 where the mesh covers the pixel; a slice
        `gbuffer[..., 0]` of a contiguous G-buffer is read in place.  Differentiable: a dense gradient of the mask's shape.
    intensity: the environment's scale per channel, 3 numbers or a tensor [3] or [B, 3]; differentiable.
    filter: 'nearest', 'bilinear' or 'trilinear'.  lod: None or a python number, lod_bias, max_level: with 'trilinear' only;
        lod=None takes the level of detail from the pixel's analytic footprint (held constant: no gradient flows through it).
    The batch size B comes from clip_to_world, mask or intensity, whichever has a leading B (they must agree); an operand
    without one is shared by the scenes.

    Returns [H, W, 3] or [B, H, W, 3]:  (1 - m) intensity E(ray), not clamped; a pixel whose ray is not valid (h.w = 0) or
    whose 1 - m is exactly 0 gives 0.  Behind a lit mesh:
        (shade_gbuffer_ibl(..., background=(0., 0., 0.), clamp=None) + environment_background(..., mask=g[..., m])).clamp(0., 1.)
    or, fused with the antialiasing and the development of the image (`resolve_image`):
        resolve_image(shade_gbuffer_ibl(..., background=(0., 0., 0.), clamp=None), add=environment_background(..., mask=g[..., m]))
    Gradients are those of torch's autograd for `lighting.environment_background` and go to the environment, clip_to_world,
    intensity and mask.  The environment's is summed with float atomics: it is not the same bits on every run, everything
    else is."""
    from .texture import CubePyramid
    who = 'environment_background'
    rows, cols, scenes, batched, n, levels, code, flags, lod, lod_bias, const = _check_background_arguments(
        environment, clip_to_world, size, mask, intensity, filter, lod, lod_bias, max_level)
    packed = isinstance(environment, CubePyramid)
    env = environment.packed if packed else environment
    _stage.require_gpu(env, 'dirt_amd.shading.%s' % who)
    matrices = clip_to_world if clip_to_world.dim() == 3 else clip_to_world[None]
    inten = _const_block(env.device, const) if const is not None else intensity.reshape(-1, 3)
    meta = (scenes, batched, rows, cols, n, levels, packed, code, flags, lod, lod_bias, max_level)
    return _EnvironmentBackground.apply(env, matrices, inten, mask, meta)


def _check_background_arguments(environment, clip_to_world, size, mask, intensity, filter, lod, lod_bias, max_level):
    """Everything `environment_background` refuses with a ValueError, on types, shapes and devices alone (no device work): ->
    (height, width, scenes, whether the output is batched, the environment's size, its levels (1 for a cube: a trilinear
    call counts them when it builds the pyramid), the filter's code, flags, lod, lod_bias, the intensity as a tuple of python
    floats or None for a tensor)."""
    from .lighting import _background_scalars
    from .texture import CubePyramid, _cube_level
    who = 'environment_background'
    rows, cols, lod_value, lod_bias = _background_scalars(size, filter, lod, lod_bias, max_level)
    if isinstance(environment, CubePyramid):
        if filter != 'trilinear':
            raise ValueError("%s: a CubePyramid is looked up with filter='trilinear', got filter=%r" % (who, filter))
        if max_level is not None:
            raise ValueError('%s: max_level applies to a cube, whose pyramid the call builds; a CubePyramid has its %d levels' % (who, environment.levels))
        if environment.channels != 3:
            raise ValueError('%s: environment has %d channels, an environment has 3' % (who, environment.channels))
        top, top_size = _cube_level(environment.size, 3, environment.levels - 1)
        if not isinstance(environment.packed, torch.Tensor) or tuple(environment.packed.shape) != (6, top + top_size * top_size * 3):
            raise ValueError('%s: environment.packed must be [6, %d], the %d levels of a %d x %d x 3 face, got %s'
                             % (who, top + top_size * top_size * 3, environment.levels, environment.size, environment.size,
                                tuple(getattr(environment.packed, 'shape', ()))))
        env, n, levels = environment.packed, environment.size, environment.levels
    else:
        if not isinstance(environment, torch.Tensor) or environment.dim() != 4 or environment.shape[0] != 6 \
                or environment.shape[1] != environment.shape[2] or 0 in environment.shape:
            raise ValueError('%s expects environment to be a cube [6, size, size, 3] or a CubePyramid, got %s'
                             % (who, tuple(getattr(environment, 'shape', ())) if isinstance(environment, torch.Tensor) else type(environment).__name__))
        if environment.shape[3] != 3:
            raise ValueError('%s: environment has %d channels, an environment has 3' % (who, environment.shape[3]))
        env, n, levels = environment, int(environment.shape[1]), 1
    _stage.check_float32('environment', env)
    _stage.check_operand('clip_to_world', clip_to_world, (4, 4), env, 'environment')
    operands = [('clip_to_world', clip_to_world, 3)]
    if mask is not None:
        _stage.check_operand('mask', mask, (rows, cols), env, 'environment')
        operands.append(('mask', mask, 3))
    const = None
    if isinstance(intensity, torch.Tensor):
        _stage.check_operand('intensity', intensity, (3,), env, 'environment')
        operands.append(('intensity', intensity, 2))
    else:
        const = tuple(_value(intensity, 3, 'intensity', env.device, None))
    scenes, batched = _stage.scene_count(who, *operands)
    flags = _lib.BACKGROUND_FOOTPRINT if filter == 'trilinear' and lod_value is None else 0
    return rows, cols, scenes, batched, n, levels, _lib.BACKGROUND_FILTERS[filter], flags, 0.0 if lod_value is None else lod_value, lod_bias, const


# ---- the developed image: supersample resolve, exposure, tone curve, sRGB encode, clamp (dirt_resolve.hip)

class _ResolveImage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, add, exposure, white, meta):
        """image, add (or None): [S H, S W, C] or [B, S H, S W, C], read in place under `_stage.rows_in_place`; exposure
        [1 or B, C], white [1 or B] or None: float32"""
        lib = _lib.load()
        scenes, batched, rows, cols, channels, factor, curve, encode, lo, hi, flags = meta
        dev = image.device
        isrc, istride = _stage.rows_in_place(image, channels)
        asrc, astride = _stage.rows_in_place(add, channels) if add is not None else (None, 0)
        exposure = exposure.contiguous()
        white = white.contiguous() if white is not None else None
        out = torch.empty(((scenes,) if batched else ()) + (rows, cols, channels), dtype=torch.float32, device=dev)
        linear = torch.empty_like(out) if any(ctx.needs_input_grad[:4]) else None   # L: all a backward pass reads
        ctx.sizes = (scenes, rows, cols, channels, factor)
        ctx.tail = (int(exposure.shape[0]), int(white.shape[0]) if white is not None else 1, curve, encode, lo, hi, flags)
        if scenes * rows * cols:
            _stage.call(lib.dirt_resolve_forward, dev, isrc.data_ptr(), _ptr(asrc), exposure.data_ptr(), _ptr(white), out.data_ptr(), _ptr(linear),
                        *ctx.sizes, istride, astride, scenes if image.dim() == 4 else 1, scenes if add is not None and add.dim() == 4 else 1, *ctx.tail)
        ctx.save_for_backward(linear, exposure, white)
        ctx.shape = tuple(image.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        linear, exposure, white = ctx.saved_tensors
        scenes, rows, cols, channels, factor = ctx.sizes
        dev = grad_out.device
        empty = not scenes * rows * cols
        want_image, want_add, want_e, want_w = ctx.needs_input_grad[:4]
        dense = grad_out.new_empty((scenes, rows * factor, cols * factor, 1))
        grad_image, grad_add = _stage.dense_grads(dense, (channels, channels), (want_image, want_add), empty)   # two tensors, never one storage
        grad_e, grad_w = _stage.grad_outputs((exposure, white), (want_e, want_w and white is not None), empty)
        if not empty:
            grad_out = grad_out.to(torch.float32).contiguous()
            nbytes = lib.dirt_resolve_scratch_bytes(*ctx.sizes) if grad_e is not None or grad_w is not None else 0
            _stage.call(lib.dirt_resolve_backward, dev, linear.data_ptr(), exposure.data_ptr(), _ptr(white), grad_out.data_ptr(), _ptr(grad_image),
                        _ptr(grad_add), _ptr(grad_e), _ptr(grad_w), _ptr(_stage.scratch(dev, nbytes)), nbytes, *ctx.sizes, *ctx.tail)
        if len(ctx.shape) == 3:   # an image shared by the scenes: summed over them, in scene order
            grad_image, grad_add = (None if g is None else (g[0] if scenes == 1 else g.sum(0)) for g in (grad_image, grad_add))
        return grad_image, grad_add, grad_e, grad_w, None


def resolve_image(image, *, add=None, factor=1, exposure=1.0, curve='linear', white=None, encode='linear', clamp=(0., 1.)):
    """The last stage of the renderer in one kernel, differentiably: what `lighting.resolve_image` computes per pixel (its
    docstring is the specification) -- `add` summed onto `image` sample by sample, `factor` x `factor` samples box-filtered
    into a pixel, exposure, a tone curve, the sRGB transfer function and the clamp -- with no image in between.

    image: float32 on the GPU, [S H, S W, C] or [B, S H, S W, C] with C in 1..4 and S = `factor`; read in place where it is
        `rgba[..., :3]` or another slice of a contiguous G-buffer.
    add: None, or a second image of exactly image's shape, read in place by the same rule: behind a lit mesh,
        resolve_image(shade_gbuffer_ibl(..., background=(0., 0., 0.), clamp=None), add=environment_background(..., mask=g[..., m]), ...)
    factor: a python int in 1..4 that divides both sides of the image; 1 develops every pixel by itself.
    exposure: the gain per channel (exposure and white balance in one): a number, C numbers, or a tensor [C] or [B, C].
    curve: 'linear', 'reinhard' (extended Reinhard; needs `white`, a positive number or a tensor [] or [B]) or 'aces' (the
        Narkowicz fit).  encode: 'linear' or 'srgb'.  clamp: (lo, hi) or None.
    The batch size B comes from image, add, exposure or white, whichever has a leading B (they must agree); an operand
    without one is shared by the scenes.

    Returns [H, W, C] or [B, H, W, C] float32.  Gradients are those of torch's autograd for `lighting.resolve_image` and go to
    image, add (a tensor of its own), exposure and white where they are tensors; the same bits on every run."""
    from .lighting import _resolve_scalars, _resolve_sizes
    who = 'resolve_image'
    bounds = _resolve_scalars(factor, curve, white, encode, clamp)
    rows, cols, channels = _resolve_sizes(image, factor)
    _stage.check_float32('image', image)
    operands = [('image', image, 4)]
    if add is not None:
        if not isinstance(add, torch.Tensor) or add.shape != image.shape:
            raise ValueError('%s: add must have the shape of image, %s, got %s' % (who, tuple(image.shape), tuple(getattr(add, 'shape', ()))))
        _stage.check_float32('add', add, image, 'image')
        operands.append(('add', add, 4))
    dev = image.device
    if isinstance(exposure, torch.Tensor):
        _stage.check_operand('exposure', exposure, (channels,), image, 'image')
        operands.append(('exposure', exposure, 2))
        gains = exposure.reshape(-1, channels)
    else:
        gains = (float(exposure),) * channels if isinstance(exposure, numbers.Real) else tuple(_value(exposure, channels, 'exposure', dev, None))
    if isinstance(white, torch.Tensor):
        if white.dim() > 1:
            raise ValueError('white must have shape [] or [B], got %s' % (tuple(white.shape),))
        _stage.check_float32('white', white, image, 'image')
        operands.append(('white', white, 1))
        point = white.reshape(-1)
    else:
        point = None if white is None else (float(white),)
    scenes, batched = _stage.scene_count(who, *operands)
    _stage.require_gpu(image, 'dirt_amd.shading.%s' % who)
    if isinstance(gains, tuple):
        gains = _const_block(dev, gains)
    if isinstance(point, tuple):
        point = _const_block(dev, point).reshape(1)
    lo, hi = bounds if bounds is not None else (0., 0.)
    meta = (scenes, batched, rows, cols, channels, int(factor), _lib.RESOLVE_CURVES[curve], _lib.RESOLVE_ENCODINGS[encode], lo, hi,
            _lib.RESOLVE_CLAMP if bounds is not None else 0)
    return _ResolveImage.apply(image, add, gains, point, meta)
