"""A texture per scene (dirt_amd.texture.sample_texture_uv_batch, mip_pyramid_batch; include/dirt_hip.h dirt_texture_*_batch*):
the batched look-up is the single-texture look-up per scene, stacked.  The references are the single-texture ones, per scene:
oracle/texture_oracle.py for 'nearest' / 'bilinear' (forward bit for bit, gradients per element within parity.TIGHT_TOL of the
mass), tests/mip_reference.py for 'trilinear' (1e-5 of the magnitude / mass); and the single-texture GPU call per scene
(forward, grad_uvs and grad_lod bit for bit; grad_textures by mass: the order of the atomics may differ)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import texture_oracle as tex_oracle
from tests import mip_reference as mr
from tests import parity
from tests.test_texture import _forward_equal, _per_element, _smooth_uv
from tests.test_texture_edges import TEX_PATCH, _tile_boxes
from tests.test_texture_mip import TOL, _bits_equal, _smooth_uv as _smooth_uv_mip
from tests.test_texture_mip_edges import _close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('repeat', 'clamp')
NAMES = ('dirt_texture_sample_batch_forward', 'dirt_texture_sample_batch_backward_image', 'dirt_texture_mip_build_batch',
         'dirt_texture_mip_collapse_batch', 'dirt_texture_sample_mip_batch_forward', 'dirt_texture_sample_mip_batch_backward')


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


# ---- refusals, before any device work (CPU) ---------------------------------------------------------------------------

def test_wrapper_refusals_with_their_text():
    """Every refusal of sample_texture_uv_batch and mip_pyramid_batch is a ValueError with a full sentence, raised on CPU and
    `meta` tensors: no device work precedes it."""
    from dirt_amd import texture as tx
    t, u = torch.zeros(3, 8, 8, 3), torch.zeros(3, 5, 6, 2)

    def refused(text, *args, **kw):
        with pytest.raises(ValueError) as e:
            tx.sample_texture_uv_batch(*args, **kw)
        assert str(e.value) == text, str(e.value)

    who = 'sample_texture_uv_batch'
    refused(who + ' expects textures to be 4D [scenes, height, width, channels], got shape (8, 8, 3)', t[0], u)
    refused(who + ' expects textures to be 4D [scenes, height, width, channels], got shape (1, 3, 8, 8, 3)', t[None], u)
    refused(who + ' expects uvs of shape [scenes, ..., 2], got (3, 5, 3)', t, torch.zeros(3, 5, 3))
    refused(who + ' expects uvs of shape [scenes, ..., 2], got (2,)', t, torch.zeros(2))
    refused(who + ': 3 scenes of textures, 2 of uvs', t, u[:2])
    refused(who + ': 3 scenes of textures, 5 of uvs', t, torch.zeros(5, 3, 2))
    for filt in ('bilinear', 'nearest'):
        for kw in ({'lod': torch.zeros(3, 5, 6)}, {'lod_bias': 0.5}, {'mask': torch.ones(3, 5, 6)}, {'max_level': 2}):
            refused("lod, lod_bias, mask and max_level apply to filter='trilinear' only (got filter=%r)" % filt, t, u, filter=filt, **kw)
    refused('lod must be a tensor shaped like uvs[..., 0] (3, 5, 6), got (5, 6)', t, u, filter='trilinear', lod=torch.zeros(5, 6))
    refused('mask must be a tensor shaped like uvs[..., 0] (3, 5, 6), got (3, 5, 6, 1)', t, u, filter='trilinear', mask=torch.ones(3, 5, 6, 1))
    refused('max_level must be a non-negative int or None, got -1', t, u, filter='trilinear', max_level=-1)
    refused("filter='trilinear' without lod takes the level of detail from neighbouring pixels: uvs must be images [..., H, W, 2], got (3, 30, 2)",
            t, torch.zeros(3, 30, 2), filter='trilinear')
    refused('mask marks the neighbours of the footprint level of detail; it does not apply with an explicit lod',
            t, u, filter='trilinear', lod=torch.zeros(3, 5, 6), mask=torch.ones(3, 5, 6))
    meta = torch.zeros(3, 5, 6, 2, device='meta')
    refused('textures and uvs must be on the same device (cpu vs meta)', t, meta)
    refused('lod and uvs must be on the same device (meta vs cpu)', t, u, filter='trilinear', lod=meta[..., 0])
    refused(who + ' runs on an MI355X only and has no CPU fallback: textures is on cpu', t, u)
    refused(who + ' runs on an MI355X only and has no CPU fallback: textures is on cpu', t, u, filter='trilinear')
    for bad, shape in ((t[0], (8, 8, 3)), (torch.zeros(8, 8), (8, 8))):
        with pytest.raises(ValueError) as e:
            tx.mip_pyramid_batch(bad)
        assert str(e.value) == 'mip_pyramid_batch expects textures to be 4D [scenes, height, width, channels], got shape %s' % (shape,)
    with pytest.raises(ValueError) as e:
        tx.mip_pyramid_batch(t)
    assert str(e.value) == 'mip_pyramid_batch runs on an MI355X only and has no CPU fallback: textures is on cpu'


def test_entry_points_refuse_bad_scenes_before_any_device_work(lib):
    """The six batched entry points: _lib.SYMBOLS names them and the library exports them; a negative scene count, a
    scenes x extent that overflows, more scenes than one launch addresses, NULL pointers and an image_rows that does not
    divide rows all return DIRT_E_INVALID_ARGUMENT with their text.  The pointers are never dereferenced."""
    from dirt_amd import _lib
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    p = ctypes.c_void_p(16)
    err = lib.dirt_texture_last_error
    FWD, BWD, BUILD, COLLAPSE, MFWD, MBWD = NAMES

    def fwd(tex=p, uvs=p, out=p, scenes=3, n=4, ht=8, wt=8, ct=3, uv_stride=2):
        return lib.dirt_texture_sample_batch_forward(tex, uvs, out, scenes, n, ht, wt, ct, uv_stride, 0, None)

    def bwd(tex=p, uvs=p, gout=p, gtex=p, guv=p, scenes=3, rows=2, cols=2, ht=8, wt=8, ct=3, uv_stride=2, guv_stride=2):
        return lib.dirt_texture_sample_batch_backward_image(tex, uvs, gout, gtex, guv, scenes, rows, cols, ht, wt, ct, uv_stride, guv_stride, 0, None)

    def build(tex=p, pyr=p, scenes=3, ht=8, wt=8, ct=3, levels=4):
        return lib.dirt_texture_mip_build_batch(tex, pyr, scenes, ht, wt, ct, levels, None)

    def collapse(gp=p, gt=p, scenes=3, ht=8, wt=8, ct=3, levels=4):
        return lib.dirt_texture_mip_collapse_batch(gp, gt, scenes, ht, wt, ct, levels, None)

    def mfwd(pyr=p, uvs=p, lod=None, mask=None, out=p, scenes=3, rows=4, cols=2, image_rows=2, ht=8, wt=8, ct=3, levels=4, uv_stride=2):
        return lib.dirt_texture_sample_mip_batch_forward(pyr, uvs, lod, mask, out, scenes, rows, cols, image_rows, ht, wt, ct, levels, uv_stride, 1, 0.0, 0, None)

    def mbwd(pyr=p, uvs=p, lod=None, mask=None, gout=p, gpyr=p, gtex=p, guv=p, glod=None, scenes=3, rows=4, cols=2, image_rows=2, ht=8, wt=8,
             ct=3, levels=4, uv_stride=2, guv_stride=2):
        return lib.dirt_texture_sample_mip_batch_backward(pyr, uvs, lod, mask, gout, gpyr, gtex, guv, glod, scenes, rows, cols, image_rows, ht, wt,
                                                          ct, levels, uv_stride, guv_stride, 1, 0.0, 0, None)

    def refused(rc, text):
        assert rc == _lib.E_INVALID_ARGUMENT, (rc, text, err())
        assert err() == text.encode(), (text, err())

    for call, who in ((fwd, FWD), (bwd, BWD), (build, BUILD), (collapse, COLLAPSE), (mfwd, MFWD), (mbwd, MBWD)):
        refused(call(scenes=-1), '%s: bad scene count (scenes=-1)' % who)
        refused(call(scenes=65536), '%s: 65536 scenes, one launch addresses at most 65535' % who)
        refused(call(scenes=1 << 40), '%s: %d scenes, one launch addresses at most 65535' % (who, 1 << 40))
    big = 1 << 30   # 2^30 x 2^30 look-ups a scene: x uv_stride x 60 000 scenes passes 2^63
    refused(fwd(scenes=60000, n=big * big), '%s: 60000 scenes of %d x 2 floats overflow' % (FWD, big * big))
    refused(bwd(scenes=60000, rows=big, cols=big), '%s: 60000 scenes of %d x 2 floats overflow' % (BWD, big * big))
    refused(mfwd(scenes=60000, rows=big, cols=big, image_rows=1), '%s: 60000 scenes of %d x 2 floats overflow' % (MFWD, big * big))
    refused(mbwd(scenes=60000, rows=big, cols=big, image_rows=1), '%s: 60000 scenes of %d x 2 floats overflow' % (MBWD, big * big))
    refused(fwd(scenes=3, n=1 << 62, uv_stride=3), '%s: 3 scenes of %d x 3 floats overflow' % (FWD, 1 << 62))      # (the extent itself)
    for call, who in ((build, BUILD), (collapse, COLLAPSE)):                  # a pyramid of 2^62 floats a scene
        refused(call(scenes=3, ht=big, wt=big, ct=4, levels=1), '%s: 3 scenes of %d x 1 floats overflow' % (who, 1 << 62))
    # the single-texture checks come first and keep their text
    refused(fwd(tex=None), FWD + ': texture / uvs is NULL')
    refused(fwd(uvs=None), FWD + ': texture / uvs is NULL')
    refused(fwd(out=None), FWD + ': out is NULL')
    refused(fwd(ht=0), '%s: bad sizes (n=4 Ht=0 Wt=8 Ct=3 uv_stride=2)' % FWD)
    refused(fwd(n=-1, scenes=-1), '%s: bad sizes (n=-1 Ht=8 Wt=8 Ct=3 uv_stride=2)' % FWD)
    refused(bwd(tex=None), BWD + ': texture / uvs is NULL')
    refused(bwd(gout=None), BWD + ': grad_out / grad_textures is NULL')
    refused(bwd(gtex=None), BWD + ': grad_out / grad_textures is NULL')
    refused(bwd(guv_stride=1), BWD + ': grad_uv_stride < 2')
    refused(bwd(rows=-1), '%s: bad pixel grid (rows=-1 cols=2)' % BWD)
    refused(bwd(rows=2, cols=1 << 31), '%s: pixel grid too large (rows=2 cols=%d)' % (BWD, 1 << 31))
    refused(build(tex=None), BUILD + ': texture / pyramid is NULL')
    refused(build(pyr=None), BUILD + ': texture / pyramid is NULL')
    refused(build(levels=5), BUILD + ': 5 levels, a 8 x 8 texture has 1..4')
    refused(collapse(gp=None), COLLAPSE + ': grad_pyramid / grad_texture is NULL')
    refused(collapse(gt=None), COLLAPSE + ': grad_pyramid / grad_texture is NULL')
    for call, who in ((mfwd, MFWD), (mbwd, MBWD)):
        refused(call(rows=4, image_rows=3), '%s: image_rows=3 does not divide rows=4' % who)
        refused(call(image_rows=0), '%s: image_rows=0 does not divide rows=4' % who)
        refused(call(pyr=None), who + ': pyramid / uvs is NULL')
        refused(call(uvs=None), who + ': pyramid / uvs is NULL')
        refused(call(scenes=-2, image_rows=3), '%s: image_rows=3 does not divide rows=4' % who)   # the order: the single-texture checks, then the scenes
    refused(mfwd(out=None), MFWD + ': out is NULL')
    refused(mbwd(gpyr=None), MBWD + ': grad_pyramid / grad_texture is NULL')
    refused(mbwd(gout=None), MBWD + ': grad_out is NULL')
    refused(mbwd(glod=p), MBWD + ': grad_lod needs lod')
    # no scenes: accepted, nothing launched
    for rc in (fwd(scenes=0), bwd(scenes=0), build(scenes=0), collapse(scenes=0), mfwd(scenes=0), mbwd(scenes=0)):
        assert rc == 0 and err() == b'', (rc, err())


# ---- helpers of the GPU tests -----------------------------------------------------------------------------------------

def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _oracle(tex, uv, g, mode, filt):
    """The per-scene oracle, stacked: forward, grad_textures, grad_uvs, mass_textures, mass_uvs."""
    out = np.stack([tex_oracle.sample_texture_uv(tex[b], uv[b], mode, filt) for b in range(len(tex))])
    grads = [tex_oracle.sample_texture_uv_grad(tex[b], uv[b], g[b], mode, filt, want_mass=True) for b in range(len(tex))]
    return (out,) + tuple(np.stack(x) for x in zip(*grads))


def _batch_and_loop(gpu, tex, uv, g, mode, filt, **kw):
    """The batched call and the single-texture call per scene on the GPU, each with its gradients: -> (out, grads), (out, grads);
    grads = [grad_textures, grad_uvs] (+ [grad_lod] with kw['lod'])."""
    from dirt_amd import texture
    lod = kw.get('lod')

    def leaves(b=None):
        xs = [tex, uv] + ([lod] if lod is not None else [])
        return [_dev(gpu, x if b is None else x[b]).requires_grad_(True) for x in xs]

    def keywords(xs, b=None):
        k = dict(kw)
        if lod is not None:
            k['lod'] = xs[2]
        if k.get('mask') is not None and b is not None:
            k['mask'] = k['mask'][b]
        return k

    xs = leaves()
    out = texture.sample_texture_uv_batch(xs[0], xs[1], mode, filt, **keywords(xs))
    grads = torch.autograd.grad(out, xs, _dev(gpu, g))
    single, sgrads = [], []
    for b in range(len(tex)):   # (leaves per scene: a gradient that came back through an index would have lost the sign of a -0)
        ys = leaves(b)
        single.append(texture.sample_texture_uv(ys[0], ys[1], mode, filt, **keywords(ys, b)))
        sgrads.append(torch.autograd.grad(single[-1], ys, _dev(gpu, g[b])))
    return (out, grads), (torch.stack(single), [torch.stack(x) for x in zip(*sgrads)])


def _same_as_the_loop(batch, loop, mass_textures, what, tol=None):
    """Per-look-up results involve no atomics: bit for bit; grad_textures by the mass of each element's terms."""
    (out, grads), (single, sgrads) = batch, loop
    assert torch.equal(out.view(torch.int32), single.view(torch.int32)), what + ': forward differs from the per-scene calls'
    for k, name in list(enumerate(('grad_textures', 'grad_uvs', 'grad_lod')))[1:len(grads)]:
        assert torch.equal(grads[k].view(torch.int32), sgrads[k].view(torch.int32)), '%s: %s differs from the per-scene calls' % (what, name)
    # (each side is within tol x mass of the exact sum, so the two are within twice that of each other)
    _close(grads[0], sgrads[0].cpu().numpy(), 2 * np.asarray(mass_textures), what + ' grad_textures against the per-scene calls',
           parity.TIGHT_TOL if tol is None else tol)


def _check_bilinear(gpu, tex, uv, g, mode, filt, what):
    """The batch against the oracle (forward bit for bit, gradients per element) and against the per-scene GPU calls -> grad_textures."""
    batch, loop = _batch_and_loop(gpu, tex, uv, g, mode, filt)
    want, want_t, want_uv, mt, muv = _oracle(tex, uv, g, mode, filt)
    _forward_equal(batch[0], want, what + ' forward')
    _per_element(batch[1][0], want_t, mt, what + ' grad_textures')
    _per_element(batch[1][1], want_uv, muv, what + ' grad_uvs')
    _same_as_the_loop(batch, loop, mt, what)
    return batch[1][0]


def _mip_reference(tex, uv, g, mode, lod=None, mask=None, **kw):
    """tests/mip_reference.py per scene, stacked: (forward, magnitude), the dict of mr.grad."""
    B = len(tex)
    pick = lambda x, b: None if x is None else x[b]
    fwd = [mr.sample(tex[b], uv[b], mode, lod=pick(lod, b), mask=pick(mask, b), magnitude=True, **kw) for b in range(B)]
    grads = [mr.grad(tex[b], uv[b], g[b], mode, lod=pick(lod, b), mask=pick(mask, b), **kw) for b in range(B)]
    return np.stack([f[0] for f in fwd]), np.stack([f[1] for f in fwd]), {k: np.stack([r[k] for r in grads]) for k in grads[0]}


def _check_trilinear(gpu, tex, uv, g, mode, what, lod=None, mask=None, mask_t=None, **kw):
    """The batch against the restatement (1e-5 of magnitude / mass) and against the per-scene GPU calls."""
    gpu_kw = dict(kw)
    if lod is not None:
        gpu_kw['lod'] = lod
    if mask is not None:
        gpu_kw['mask'] = _dev(gpu, mask) if mask_t is None else mask_t
    batch, loop = _batch_and_loop(gpu, tex, uv, g, mode, 'trilinear', **gpu_kw)
    want, mag, r = _mip_reference(tex, uv, g, mode, lod=lod, mask=mask, **kw)
    _close(batch[0], want, mag, what + ' forward', TOL)
    _close(batch[1][0], r['grad_texture'], r['mass_texture'], what + ' grad_textures', TOL)
    _close(batch[1][1], r['grad_uvs'], r['mass_uvs'], what + ' grad_uvs', TOL)
    if lod is not None:
        _close(batch[1][2], r['grad_lod'], r['mass_lod'], what + ' grad_lod', TOL)
    _same_as_the_loop(batch, loop, r['mass_texture'], what, TOL)


# ---- 1. scenes do not leak --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('filt', ['bilinear', 'nearest'])
def test_scenes_do_not_leak(gpu, ct, mode, filt):
    """Three scenes of 24 x 40 look-ups: 24 is no multiple of 16, so tiles laid over the stacked rows would mix two scenes in
    the last tile row of each.  Scene b's texture is random + 10 b: a read from, or a gradient into, the wrong scene is off
    by about 10, not by rounding."""
    rng = np.random.default_rng(200 + ct)
    tex = (rng.uniform(-1, 1, (3, 20, 31, ct)) + 10 * np.arange(3).reshape(3, 1, 1, 1)).astype(np.float32)
    uv = rng.uniform(-1.5, 2.5, (3, 24, 40, 2)).astype(np.float32)
    g = rng.standard_normal((3, 24, 40, ct)).astype(np.float32)
    _check_bilinear(gpu, tex, uv, g, mode, filt, 'ct=%d %s %s' % (ct, mode, filt))


# ---- 2. the patch path per scene --------------------------------------------------------------------------------------

def _quarter_uv(b, H, W, seed):
    """A smooth field (test_texture._smooth_uv) squeezed into quarter b of its texture: (u, v) in [x0 + 0.04, x0 + 0.44]."""
    f = _smooth_uv(1, H, W, 1.0, seed, seam=False)[0].astype(np.float64)
    f = (f - f.min((0, 1))) / (f.max((0, 1)) - f.min((0, 1)))
    return (np.array([0.5 * (b % 2), 0.5 * (b // 2)]) + 0.04 + 0.4 * f).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_patch_path_per_scene(gpu, ct):
    """Three smooth coordinate images, each inside another quarter of its texture: every tile sums in the LDS patch
    (_tile_boxes asserts it), and the patch, its box and its flush are one scene's -- grad_textures[b] is exactly 0 outside
    scene b's quarter and the oracle's inside.  Again with scene 1's coordinates random: its tiles scatter atomics straight
    into scene 1's gradient while scenes 0 and 2 keep the patch."""
    rng = np.random.default_rng(210 + ct)
    Ht, Wt, H, W = 40, 48, 32, 48
    tex = rng.uniform(-1, 1, (3, Ht, Wt, ct)).astype(np.float32)
    g = rng.standard_normal((3, H, W, ct)).astype(np.float32)
    smooth = np.stack([_quarter_uv(b, H, W, 5 + b) for b in range(3)])
    mixed = smooth.copy()
    mixed[1] = rng.uniform(-0.5, 1.5, (H, W, 2)).astype(np.float32)
    for uv, random_scene in ((smooth, None), (mixed, 1)):
        for mode in MODES:
            for b in range(3):
                fits = np.prod(_tile_boxes(uv[b], Ht, Wt, mode, 'bilinear', H, W), axis=-1) <= TEX_PATCH
                assert (not fits.any()) if b == random_scene else fits.all(), (b, mode)
            gt = _check_bilinear(gpu, tex, uv, g, mode, 'bilinear', 'quarters ct=%d %s random=%s' % (ct, mode, random_scene))
            for b in range(3):
                if b == random_scene:
                    continue
                r0, c0 = (b // 2) * Ht // 2, (b % 2) * Wt // 2
                outside = torch.ones(Ht, Wt, dtype=torch.bool, device=gpu)
                outside[r0:r0 + Ht // 2, c0:c0 + Wt // 2] = False
                assert bool((gt[b][outside] == 0).all()) and bool((gt[b][~outside] != 0).any()), (b, mode)


# ---- 3. flat lists ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 4])
def test_flat_lists(gpu, ct):
    """[3, 300, 2]: 300 is no multiple of 256, so a 256 x 1 run over the concatenated lists would straddle two scenes."""
    rng = np.random.default_rng(220 + ct)
    tex = (rng.uniform(-1, 1, (3, 16, 32, ct)) + 10 * np.arange(3).reshape(3, 1, 1, 1)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (3, 300, 2)).astype(np.float32)
    uv[:, :150] = np.stack([0.1 + 0.3 * np.linspace(0, 1, 150), 0.8 - 0.25 * np.linspace(0, 1, 150)], -1)   # a run that takes the patch
    g = rng.standard_normal((3, 300, ct)).astype(np.float32)
    lod = rng.uniform(-0.5, 5.5, (3, 300)).astype(np.float32)
    for mode in MODES:
        _check_bilinear(gpu, tex, uv, g, mode, 'bilinear', 'flat ct=%d %s' % (ct, mode))
        _check_trilinear(gpu, tex, uv, g, mode, 'flat trilinear ct=%d %s' % (ct, mode), lod=lod, lod_bias=0.25)


# ---- 4. in place from a G-buffer, guards around every output ----------------------------------------------------------

def _guarded(gpu, shape, guard=64):
    """A NaN-filled output of `shape` between `guard` NaN floats on each side -> (buffer, operand)."""
    size = int(np.prod(shape))
    buf = torch.full((guard + size + guard,), float('nan'), device=gpu)
    return buf, buf[guard:guard + size].view(shape)


def _guards_intact(buf, shape, guard=64):
    size = int(np.prod(shape))
    return bool(buf[:guard].isnan().all()) and bool(buf[guard + size:].isnan().all())


@pytest.mark.gpu
@pytest.mark.parametrize('first,channels', [(1, 7), (2, 6)])
@pytest.mark.parametrize('ct', [3, 4])
def test_in_place_from_a_gbuffer(gpu, lib, first, channels, ct):
    """(u, v) in channels first : first + 2 of a [2, 24, 40, channels] G-buffer -- 7: an odd stride, the scalar pair load; 6 with
    first = 2: pairs on 8-byte boundaries -- and the mask in channel 0, read in place by the wrapper (data pointers asserted).
    Through the C ABI the gradients of both filters are written between NaN guards, grad_uvs in place into a G-buffer-shaped
    buffer (grad_uv_stride = channels) whose other channels must stay NaN; grad_textures and the scratch pyramid start as NaN
    and must come back fully written."""
    from dirt_amd import rasterise_ops as ops, texture
    from dirt_amd.texture import _pairs_in_place, _scalars_in_place
    B, H, W, Ht, Wt = 2, 24, 40, 32, 64
    rng = np.random.default_rng(230 + channels + ct)
    tex = (rng.uniform(-1, 1, (B, Ht, Wt, ct)) + 10 * np.arange(B).reshape(B, 1, 1, 1)).astype(np.float32)
    gbuf = rng.uniform(-0.3, 1.3, (B, H, W, channels)).astype(np.float32)
    gbuf[..., first:first + 2] = _smooth_uv_mip(B, H, W, 3.0, 7)
    gbuf[..., 0] = (np.add.outer(np.arange(H) // 5, np.arange(W) // 7) % 2)[None]
    uv, mask = np.ascontiguousarray(gbuf[..., first:first + 2]), np.ascontiguousarray(gbuf[..., 0])
    assert min(_lod_distance(uv, Ht, Wt, mode, mask=mask)[0] for mode in MODES) >= 0.2
    g = rng.standard_normal((B, H, W, ct)).astype(np.float32)
    t, gb, g_t = _dev(gpu, tex), _dev(gpu, gbuf), _dev(gpu, g)
    src, stride = _pairs_in_place(gb[..., first:first + 2])
    assert stride == channels and src.data_ptr() == gb.data_ptr() + 4 * first
    m_src, m_stride = _scalars_in_place(gb[..., 0])
    assert m_stride == channels and m_src.data_ptr() == gb.data_ptr()
    stream = ops._stream_handle(gpu)
    n = H * W

    def done(rc):
        assert rc == 0, (rc, lib.dirt_texture_last_error())
        torch.cuda.synchronize()

    for mode in MODES:
        flags = {'repeat': 0, 'clamp': 1}[mode]
        what = 'channels %d:%d of %d ct=%d %s' % (first, first + 2, channels, ct, mode)
        # bilinear: the wrapper's forward in place, the C ABI's forward and backward between guards
        want, want_t, want_uv, mt, muv = _oracle(tex, uv, g, mode, 'bilinear')
        _forward_equal(texture.sample_texture_uv_batch(t, gb[..., first:first + 2], mode), want, what + ' wrapper forward')
        obuf, out = _guarded(gpu, (B, H, W, ct))
        done(lib.dirt_texture_sample_batch_forward(t.data_ptr(), src.data_ptr(), out.data_ptr(), B, n, Ht, Wt, ct, channels, flags, stream))
        _forward_equal(out, want, what + ' forward')
        tbuf, gtex = _guarded(gpu, tex.shape)
        ubuf, ggb = _guarded(gpu, gbuf.shape)
        done(lib.dirt_texture_sample_batch_backward_image(t.data_ptr(), src.data_ptr(), g_t.data_ptr(), gtex.data_ptr(), ggb.data_ptr() + 4 * first,
                                                          B, H, W, Ht, Wt, ct, channels, channels, flags, stream))
        _per_element(gtex, want_t, mt, what + ' grad_textures')
        _per_element(ggb[..., first:first + 2], want_uv, muv, what + ' grad_uvs')
        assert bool(ggb[..., :first].isnan().all()) and bool(ggb[..., first + 2:].isnan().all()), what + ': wrote other channels'
        assert _guards_intact(obuf, out.shape) and _guards_intact(tbuf, tex.shape) and _guards_intact(ubuf, gbuf.shape), what
        # trilinear from the footprint, the mask in place
        want, mag, r = _mip_reference(tex, uv, g, mode, mask=mask)
        got = texture.sample_texture_uv_batch(t, gb[..., first:first + 2], mode, 'trilinear', mask=gb[..., 0])
        _close(got, want, mag, what + ' trilinear wrapper forward', TOL)
        levels = mr.level_count(Ht, Wt)
        floats = sum(p.size for p in mr.pyramid(tex[0]))
        pbuf, pyr = _guarded(gpu, (B, floats))
        done(lib.dirt_texture_mip_build_batch(t.data_ptr(), pyr.data_ptr(), B, Ht, Wt, ct, levels, stream))
        obuf, out = _guarded(gpu, (B, H, W, ct))
        done(lib.dirt_texture_sample_mip_batch_forward(pyr.data_ptr(), src.data_ptr(), None, m_src.data_ptr(), out.data_ptr(), B, H, W, H, Ht, Wt, ct,
                                                       levels, channels, channels, 0.0, flags, stream))
        _close(out, want, mag, what + ' trilinear forward', TOL)
        sbuf, scratch = _guarded(gpu, (B, floats))
        tbuf, gtex = _guarded(gpu, tex.shape)
        ubuf, ggb = _guarded(gpu, gbuf.shape)
        done(lib.dirt_texture_sample_mip_batch_backward(pyr.data_ptr(), src.data_ptr(), None, m_src.data_ptr(), g_t.data_ptr(), scratch.data_ptr(),
                                                        gtex.data_ptr(), ggb.data_ptr() + 4 * first, None, B, H, W, H, Ht, Wt, ct, levels, channels,
                                                        channels, channels, 0.0, flags, stream))
        _close(gtex, r['grad_texture'], r['mass_texture'], what + ' trilinear grad_textures', TOL)
        _close(ggb[..., first:first + 2], r['grad_uvs'], r['mass_uvs'], what + ' trilinear grad_uvs', TOL)
        assert bool(scratch.isfinite().all()), what + ': the scratch pyramid was not cleared'
        assert bool(ggb[..., :first].isnan().all()) and bool(ggb[..., first + 2:].isnan().all()), what + ': wrote other channels'
        for buf, shape in ((pbuf, pyr.shape), (obuf, out.shape), (sbuf, scratch.shape), (tbuf, tex.shape), (ubuf, gbuf.shape)):
            assert _guards_intact(buf, shape), what


# ---- 5. trilinear from the footprint ----------------------------------------------------------------------------------

def _lod_distance(uv, ht, wt, mode, mask=None, lod_bias=0.0):
    """The distance of the reference's lambda from the nearest integer, over the pixels that count (log2f may be an ulp off)."""
    lam = np.stack([mr.footprint_lod(uv[b], ht, wt, mode, None if mask is None else mask[b], lod_bias) for b in range(len(uv))])
    keep = np.ones(lam.shape, bool) if mask is None else mask != 0
    return float(np.abs(lam - np.rint(lam))[keep].min()), float(lam[keep].min()), float(lam[keep].max())


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('scale,seed', [(1.5, 1), (3.0, 2), (6.0, 3)])
@pytest.mark.parametrize('mode', MODES)
def test_trilinear_from_the_footprint(gpu, ct, scale, seed, mode):
    """B = 3 smooth images over 32 x 64 textures, lambda 1.2 to 3.3 with the scale and at least 0.2 from an integer (asserted, so
    that a log2f one ulp off cannot change a level): plain, with lod_bias, with max_level = 2 and with a checker mask read in
    place from channel 0 of a G-buffer.  The footprint of scene b is scene b's alone; no element is left out."""
    B, H, W, Ht, Wt = 3, 24, 40, 32, 64
    rng = np.random.default_rng(240 + ct)
    tex = (rng.uniform(-1, 1, (B, Ht, Wt, ct)) + 10 * np.arange(B).reshape(B, 1, 1, 1)).astype(np.float32)
    uv = _smooth_uv_mip(B, H, W, scale, seed)
    g = rng.standard_normal((B, H, W, ct)).astype(np.float32)
    d, lo, hi = _lod_distance(uv, Ht, Wt, mode)
    assert d >= 0.2 and {1.5: 1, 3.0: 2, 6.0: 3}[scale] + 0.2 <= lo <= hi <= {1.5: 1, 3.0: 2, 6.0: 3}[scale] + 0.27, (d, lo, hi)
    what = 'ct=%d scale=%g %s' % (ct, scale, mode)
    _check_trilinear(gpu, tex, uv, g, mode, what)
    assert _lod_distance(uv, Ht, Wt, mode, lod_bias=0.5)[0] >= 0.2
    _check_trilinear(gpu, tex, uv, g, mode, what + ' lod_bias', lod_bias=0.5)
    _check_trilinear(gpu, tex, uv, g, mode, what + ' max_level', max_level=2)
    gbuf = np.zeros((B, H, W, 6), np.float32)
    gbuf[..., 1:3] = uv
    gbuf[..., 0] = (np.add.outer(np.arange(H) // 3, np.arange(W) // 4) % 2)[None]
    assert _lod_distance(uv, Ht, Wt, mode, mask=gbuf[..., 0])[0] >= 0.2
    gb = _dev(gpu, gbuf)
    _check_trilinear(gpu, tex, uv, g, mode, what + ' mask', mask=gbuf[..., 0], mask_t=gb[..., 0])


@pytest.mark.gpu
def test_trilinear_with_two_images_per_scene(gpu):
    """uvs [2, 2, 24, 40, 2]: two images per scene, image_rows = 24 < rows = 48; the footprint stays inside each image."""
    rng = np.random.default_rng(250)
    tex = (rng.uniform(-1, 1, (2, 32, 64, 3)) + 10 * np.arange(2).reshape(2, 1, 1, 1)).astype(np.float32)
    uv = np.stack([_smooth_uv_mip(2, 24, 40, s, 4 + i) for i, s in enumerate((1.5, 6.0))])
    g = rng.standard_normal((2, 2, 24, 40, 3)).astype(np.float32)
    for mode in MODES:
        assert _lod_distance(uv, 32, 64, mode)[0] >= 0.2
        _check_trilinear(gpu, tex, uv, g, mode, 'two images per scene ' + mode)


# ---- 6. pyramids ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 32, 64, 1), (3, 32, 64, 3), (3, 32, 64, 4), (3, 32, 64, 5), (2, 6, 9, 2), (3, 256, 128, 3)])
def test_pyramids(gpu, shape):
    """mip_pyramid_batch bit for bit against mip_reference.pyramid per scene (32 x 64: the block kernel alone; 6 x 9: one level;
    256 x 128: the top kernel too, a workgroup per scene), the levels views of one scene-major buffer, and its backward against
    mip_reference.collapse."""
    from dirt_amd import texture
    rng = np.random.default_rng(sum(shape))
    tex = rng.uniform(-1, 1, shape).astype(np.float32)
    t = _dev(gpu, tex).requires_grad_(True)
    levels = texture.mip_pyramid_batch(t)
    want = [mr.pyramid(tex[b]) for b in range(shape[0])]
    assert len(levels) == len(want[0]) == mr.level_count(shape[1], shape[2])
    off = 0
    floats = sum(p.size for p in want[0])
    for k, lv in enumerate(levels):
        _bits_equal(lv, np.stack([w[k] for w in want]), 'level %d of %s' % (k, shape))
        assert lv.data_ptr() == levels[0].data_ptr() + 4 * off and lv.stride(0) == floats, 'level %d is not a view of the packed buffer' % k
        off += want[0][k].size
    assert len(texture.mip_pyramid_batch(t, max_level=1)) == min(2, len(levels))
    gs = [rng.standard_normal(tuple(lv.shape)).astype(np.float32) for lv in levels]
    gt, = torch.autograd.grad(levels, [t], [_dev(gpu, x) for x in gs])

    def factor(k):
        return 0.25 if (want[0][k].shape[0] > 1 and want[0][k].shape[1] > 1) else 0.5
    for b in range(shape[0]):
        grad = mr.collapse([x[b].astype(np.float64) for x in gs], factor)
        mass = mr.collapse([np.abs(x[b]).astype(np.float64) for x in gs], factor)
        _close(gt[b], grad, mass, 'pyramid backward of %s, scene %d' % (shape, b), TOL)


# ---- 7. one scene and none --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['nearest', 'bilinear', 'trilinear'])
def test_one_scene_is_the_single_texture_function(gpu, filt):
    rng = np.random.default_rng(260)
    tex = rng.uniform(-1, 1, (1, 32, 64, 3)).astype(np.float32)
    uv = _smooth_uv_mip(1, 24, 40, 3.0, 9)
    g = rng.standard_normal((1, 24, 40, 3)).astype(np.float32)
    cases = [{}] if filt != 'trilinear' else [{}, {'lod': rng.uniform(-0.5, 5.5, (1, 24, 40)).astype(np.float32)}]
    for kw in cases:
        batch, loop = _batch_and_loop(gpu, tex, uv, g, 'repeat', filt, **kw)
        mass = np.stack([mr.grad(tex[0], uv[0], g[0], 'repeat', **kw)['mass_texture']]) if filt == 'trilinear' else \
            _oracle(tex, uv, g, 'repeat', filt)[3]
        _same_as_the_loop(batch, loop, mass, 'B = 1 %s %s' % (filt, sorted(kw)), TOL if filt == 'trilinear' else None)


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['nearest', 'bilinear', 'trilinear'])
def test_no_scenes(gpu, filt):
    from dirt_amd import texture
    t = torch.zeros(0, 8, 16, 3, device=gpu, requires_grad=True)
    for shape in ((0, 5, 6, 2), (0, 7, 2)):
        u = torch.zeros(shape, device=gpu, requires_grad=True)
        kw = {'lod': torch.zeros(shape[:-1], device=gpu)} if filt == 'trilinear' and len(shape) == 3 else {}
        out = texture.sample_texture_uv_batch(t, u, 'repeat', filt, **kw)
        assert out.shape == shape[:-1] + (3,) and out.dtype == torch.float32 and out.device == t.device
        gt, gu = torch.autograd.grad(out, [t, u], torch.zeros_like(out))
        assert gt.shape == t.shape and gu.shape == u.shape
    levels = texture.mip_pyramid_batch(t)
    assert [tuple(lv.shape) for lv in levels] == [(0, 8, 16, 3), (0, 4, 8, 3), (0, 2, 4, 3), (0, 1, 2, 3), (0, 1, 1, 3)]


# ---- 8. the forward past the grid cap ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_forward_past_the_grid_cap(gpu):
    """2 scenes of 2049 x 2048 = 4 194 304 + 2 048 look-ups: past the 16 384 workgroups of 256 lanes a launch is capped at, so
    each scene's last 2 048 are the second turn of the grid-stride loop -- in its own scene.  Coordinates repeat a table of
    4 099 pairs per scene (a prime), so the oracle runs on the tables."""
    from dirt_amd import texture
    rng = np.random.default_rng(270)
    n, period = 2049 * 2048, 4099
    tex = (rng.uniform(-1, 1, (2, 13, 17, 1)) + 10 * np.arange(2).reshape(2, 1, 1, 1)).astype(np.float32)
    table = rng.uniform(-0.6, 1.6, (2, period, 2)).astype(np.float32)
    which = torch.arange(n, device=gpu) % period
    out = texture.sample_texture_uv_batch(_dev(gpu, tex), _dev(gpu, table)[:, which], 'repeat', 'bilinear')
    assert out.shape == (2, n, 1)
    want = np.stack([tex_oracle.sample_texture_uv(tex[b], table[b], 'repeat', 'bilinear') for b in range(2)])
    assert torch.equal(out.view(torch.int32), _dev(gpu, want).view(torch.int32)[:, which]), 'past the grid cap: differs from the oracle'


# ---- 9. captured in a graph -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['nearest', 'bilinear', 'trilinear'])
def test_a_captured_batch_lookup_and_backward_replay_on_new_textures(gpu, filt):
    """The batched look-up and its backward make no host synchronisation and clear with the library's own kernel: captured with
    torch.cuda.graph and replayed three times on textures rewritten in place, every replay equals the reference for that
    texture, and the texels no look-up touches (u, v < 0.7) come back 0 on every replay."""
    from dirt_amd import texture
    rng = np.random.default_rng(280)
    B, Ht, Wt, ct = 3, 32, 28, 3
    tex = rng.uniform(-1, 1, (B, Ht, Wt, ct)).astype(np.float32)
    uv = np.stack([np.concatenate([_smooth_uv(1, 12, 40, 0.5, 4 + b, seam=False)[0], rng.uniform(0.1, 0.65, (12, 40, 2)).astype(np.float32)])
                   for b in range(B)])
    lod = rng.uniform(-0.5, 2.5, uv.shape[:-1]).astype(np.float32)
    g = rng.standard_normal(uv.shape[:-1] + (ct,)).astype(np.float32)
    t, u, g_t = _dev(gpu, tex), _dev(gpu, uv), _dev(gpu, g)
    kw = {'lod': _dev(gpu, lod)} if filt == 'trilinear' else {}

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (t, u)]
        out = texture.sample_texture_uv_batch(leaves[0], leaves[1], 'repeat', filt, **kw)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, g_t))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, gt_g, gu_g = step()
    for k in range(3):
        tex_k = (rng.uniform(-1, 1, tex.shape) + 10 * np.arange(B).reshape(B, 1, 1, 1)).astype(np.float32)
        with torch.no_grad():
            t.copy_(_dev(gpu, tex_k))
        graph.replay()
        torch.cuda.synchronize()
        if filt == 'trilinear':
            want, mag, r = _mip_reference(tex_k, uv, g, 'repeat', lod=lod)
            _close(out_g, want, mag, 'replay %d forward' % k, TOL)
            _close(gt_g, r['grad_texture'], r['mass_texture'], 'replay %d grad_textures' % k, TOL)
            _close(gu_g, r['grad_uvs'], r['mass_uvs'], 'replay %d grad_uvs' % k, TOL)
            untouched = r['mass_texture'] == 0
        else:
            want, want_t, want_uv, mt, muv = _oracle(tex_k, uv, g, 'repeat', filt)
            _forward_equal(out_g, want, 'replay %d forward' % k)
            _per_element(gt_g, want_t, mt, 'replay %d grad_textures' % k)
            _per_element(gu_g, want_uv, muv, 'replay %d grad_uvs' % k)
            untouched = mt == 0
        assert all(untouched[b].sum() >= 10 * ct for b in range(B)) and bool((gt_g[torch.from_numpy(untouched).to(gpu)] == 0).all())


# ---- 10. what the wrapper converts ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'trilinear'])
def test_wrapper_conversions(gpu, filt):
    """The kernels see contiguous float32: textures held as [B, C, Ht, Wt] and permuted to channels-last, float64 operands
    (float64 gradients back), and requires_grad on one operand only."""
    from dirt_amd import texture
    rng = np.random.default_rng(290)
    B, Ht, Wt, ct, H, W = 2, 32, 64, 3, 24, 40
    tex = (rng.uniform(-1, 1, (B, Ht, Wt, ct)) + 10 * np.arange(B).reshape(B, 1, 1, 1)).astype(np.float32)
    uv = _smooth_uv_mip(B, H, W, 3.0, 11)
    g = rng.standard_normal((B, H, W, ct)).astype(np.float32)
    assert _lod_distance(uv, Ht, Wt, 'repeat')[0] >= 0.2
    if filt == 'trilinear':
        want, mag, r = _mip_reference(tex, uv, g, 'repeat')
        want_t, want_uv, mt, muv = r['grad_texture'], r['grad_uvs'], r['mass_texture'], r['mass_uvs']
    else:
        want, want_t, want_uv, mt, muv = _oracle(tex, uv, g, 'repeat', filt)
        mag = np.abs(want)

    tol = TOL if filt == 'trilinear' else parity.TIGHT_TOL

    def check(out, gt, gu, what):
        assert out.dtype == torch.float32
        _close(out, want, mag, what + ' forward', TOL if filt == 'trilinear' else 0.0)   # (bilinear: bit for bit)
        if gt is not None:
            _close(gt, want_t, mt, what + ' grad_textures', tol)
        if gu is not None:
            _close(gu, want_uv, muv, what + ' grad_uvs', tol)

    held = _dev(gpu, tex.transpose(0, 3, 1, 2)).requires_grad_(True)     # [B, C, Ht, Wt]
    t, u = held.permute(0, 2, 3, 1), _dev(gpu, uv).requires_grad_(True)
    assert not t.is_contiguous()
    out = texture.sample_texture_uv_batch(t, u, 'repeat', filt)
    gt, gu = torch.autograd.grad(out, [held, u], _dev(gpu, g))
    check(out, gt.permute(0, 2, 3, 1), gu, 'channels-first textures')
    t, u = _dev(gpu, tex).double().requires_grad_(True), _dev(gpu, uv).double().requires_grad_(True)
    out = texture.sample_texture_uv_batch(t, u, 'repeat', filt)
    gt, gu = torch.autograd.grad(out, [t, u], _dev(gpu, g))
    assert gt.dtype == torch.float64 and gu.dtype == torch.float64
    check(out, gt, gu, 'float64')
    t, u = _dev(gpu, tex).requires_grad_(True), _dev(gpu, uv)
    out = texture.sample_texture_uv_batch(t, u, 'repeat', filt)
    check(out, torch.autograd.grad(out, [t], _dev(gpu, g))[0], None, 'textures only')
    t, u = _dev(gpu, tex), _dev(gpu, uv).requires_grad_(True)
    out = texture.sample_texture_uv_batch(t, u, 'repeat', filt)
    check(out, None, torch.autograd.grad(out, [u], _dev(gpu, g))[0], 'uvs only')


# ---- 12. the example --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_example_descends_in_every_scene(gpu):
    """examples/textured_batch.py at a small frame: rasterise_batch_deferred with a shader that looks three textures up in one
    launch; the loss is lower at every step and every scene's loss falls."""
    spec = importlib.util.spec_from_file_location('example_textured_batch', os.path.join(ROOT, 'examples', 'textured_batch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(scenes=3, height=64, width=64, steps=5, device=gpu, quiet=True)
    assert losses.shape == (5, 3) and np.isfinite(losses).all()
    total = losses.mean(1)
    assert all(total[k + 1] < total[k] for k in range(4)), total
    assert (losses[-1] < losses[0]).all(), losses
