"""Edges of the trilinear look-up (dirt_texture_mip.hip) that tests/test_texture_mip.py leaves out: the restatement
tests/mip_reference.py against an independent float64 autograd version of DESIGN.md §7, the C entry points' argument
checks, non-finite input, texel and level edges, layouts, the sizes where the kernels' grids and loops stride, and
rasterise_deferred with a trilinear shader."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mip_reference as mr

TOL = 1e-5   # per element, relative to the L1 mass of the element's terms (forward: to the value's magnitude)


def _np64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def _close(got, want, mass, what, tol=TOL):
    """|got - want| <= tol * mass per element; non-finite values (NaN or +-inf) exactly where `want` or `mass` is not
    finite; where the mass is 0, got must be 0."""
    got, want, mass = _np64(got), np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape == mass.shape, (what, got.shape, want.shape, mass.shape)
    bad_w = ~(np.isfinite(want) & np.isfinite(mass))
    bad_g = ~np.isfinite(got)
    assert np.array_equal(bad_w, bad_g), '%s: non-finite values in different places (%d expected, %d got; first mismatch at %s)' % (
        what, bad_w.sum(), bad_g.sum(), np.argwhere(bad_w != bad_g)[:1].tolist())
    ok = ~bad_w
    err, lim = np.abs(got - want)[ok], tol * mass[ok]
    if err.size and not np.all(err <= lim):
        worst = int(np.argmax(err - lim))
        raise AssertionError('%s: %d of %d elements outside %g * mass; worst err %g at mass %g (value %g)' % (
            what, int(np.sum(err > lim)), err.size, tol, err[worst], mass[ok][worst], want[ok][worst]))


# ---- the restatement against DESIGN.md §7 written again in float64 torch, with autograd (CPU) --------------------------

def _spec_dims(ht, wt, max_level):
    """§7 (1): level k + 1 exists while level k is not 1 x 1, each of its dimensions is even or 1, and k + 1 <= max_level."""
    dims = [(ht, wt)]
    while True:
        h, w = dims[-1]
        if (h, w) == (1, 1) or (h > 1 and h % 2) or (w > 1 and w % 2) or (max_level is not None and len(dims) > max_level):
            return dims
        dims.append((max(h // 2, 1), max(w // 2, 1)))


def _r32(x):
    """x rounded to float32, with the gradient of x: one float32 operation of the kernels, differentiated in float64."""
    return x + (x.to(torch.float32).to(torch.float64) - x).detach()


def _spec_lookup(tex, uv, lam, mode, max_level):
    """§7 (1, 2, 4): tex [Ht, Wt, C], uv [n, 2], lam [n] (lod + lod_bias, or the footprint's) float64 -> [n, C]."""
    ht, wt, ct = tex.shape
    dims = _spec_dims(ht, wt, max_level)
    levels = [tex]
    for h, w in dims[1:]:
        t = levels[-1]
        kh, kw = t.shape[0] // h, t.shape[1] // w
        levels.append(t.reshape(h, kh, w, kw, ct).mean(dim=(1, 3)))          # 2 x 2 or 2 x 1 means
    u, v = uv[:, 0], uv[:, 1]
    if mode == 'repeat':                                                      # uv_to_index, in float32
        row, col = _r32(_r32(v - torch.floor(v)) * ht), _r32(_r32(u - torch.floor(u)) * wt)
    else:                                                                     # clip_by_value: gradient 1 on [0, 1]
        row = _r32(torch.where(v < 0, torch.zeros_like(v), torch.where(v > 1, torch.ones_like(v), v)) * ht)
        col = _r32(torch.where(u < 0, torch.zeros_like(u), torch.where(u > 1, torch.ones_like(u), u)) * wt)
    samples = []
    for k, (h, w) in enumerate(dims):
        rk, ck = row, col
        if k:
            sr, sc = ht / h, wt / w
            rk, ck = _r32(_r32(row - (sr - 1) * 0.5) / sr), _r32(_r32(col - (sc - 1) * 0.5) / sc)
            rk = torch.where(rk < 0, torch.zeros_like(rk), rk)                 # max(., 0): no gradient where it clamps
            ck = torch.where(ck < 0, torch.zeros_like(ck), ck)
        fr0, fc0 = torch.floor(rk).detach(), torch.floor(ck).detach()
        fr, fc = (rk - fr0)[:, None], (ck - fc0)[:, None]
        r0, c0 = fr0.clamp(0, h - 1).long(), fc0.clamp(0, w - 1).long()
        r1, c1 = (r0 + 1).clamp(max=h - 1), (c0 + 1).clamp(max=w - 1)         # the last-texel rule
        t = levels[k]
        samples.append(t[r0, c0] * (1 - fc) * (1 - fr) + t[r0, c1] * fc * (1 - fr) + t[r1, c0] * (1 - fc) * fr + t[r1, c1] * fc * fr)
    top = float(len(dims) - 1)
    c = torch.where(lam > 0, torch.where(lam < top, lam, torch.full_like(lam, top)), torch.zeros_like(lam))
    l = torch.floor(c).detach().long()
    f = (c - l)[:, None]
    stack = torch.stack(samples)                                              # [L, n, C]
    n = torch.arange(len(lam))
    return (1 - f) * stack[l, n] + f * stack[(l + 1).clamp(max=len(dims) - 1), n]


def _spec_grads(tex, uv, g, mode, lam, lod_given, max_level):
    t = torch.from_numpy(tex.astype(np.float64)).requires_grad_(True)
    u = torch.from_numpy(uv.reshape(-1, 2).astype(np.float64)).requires_grad_(True)
    lt = torch.from_numpy(lam.reshape(-1).astype(np.float64)).requires_grad_(lod_given)
    out = _spec_lookup(t, u, lt, mode, max_level)
    leaves = [t, u] + ([lt] if lod_given else [])
    grads = torch.autograd.grad(out, leaves, torch.from_numpy(g.reshape(out.shape).astype(np.float64)))
    return out.detach().numpy(), grads


def _edge_values(n0):
    """Coordinates on level-0 and coarser texel edges of an axis of n0 texels, within half a coarse texel of the border,
    0, -0.0, 1, just below 1 and whole numbers."""
    vals = [0.0, -0.0, 1.0, 1.0 - 2 ** -24, 2.0, -1.0, 3.0, 0.5]
    s = 1
    while s <= n0:
        vals += [(j * s + (s - 1) * 0.5) / n0 for j in range(0, n0 // s + 1, max(1, n0 // s // 3))]
        vals += [0.25 * (s - 1) / n0, 0.5 * (s - 1) / n0]                     # index_k < 0: the max clamps
        s *= 2
    return vals


def _lod_values(levels):
    vals = [0.0, -0.0, -0.5, 0.5, 1.5, float(levels - 1), levels - 0.5, float(levels), levels + 3.0, -7.0]
    for k in range(1, levels + 1):
        vals += [float(k), float(np.nextafter(np.float32(k), np.float32(-np.inf)))]
    return vals


@pytest.mark.parametrize('shape', [(8, 2), (2, 16), (480, 640), (1, 1), (12, 20), (64, 32)])
def test_restatement_gradients_are_the_spec_under_autograd(shape):
    """mr.grad against DESIGN.md §7 restated in float64 torch (above), its gradients from autograd: every element of
    grad_texture, grad_uvs and grad_lod, in both modes, at several max_level, with random, integer and out-of-range lods."""
    rng = np.random.default_rng(sum(shape))
    ht, wt = shape
    for ct in (1, 3):
        tex = rng.uniform(-1, 1, (ht, wt, ct)).astype(np.float32)
        for max_level in (None, 0, 1, 3):
            L = mr.level_count(ht, wt, max_level)
            assert L == len(_spec_dims(ht, wt, max_level))
            n = 300
            uv = rng.uniform(-1.3, 2.3, (n, 2)).astype(np.float32)
            ev_u, ev_v = _edge_values(wt), _edge_values(ht)
            uv[:40, 0] = rng.choice(ev_u, 40)
            uv[20:60, 1] = rng.choice(ev_v, 40)
            lod = rng.uniform(-1.5, L + 1.5, n).astype(np.float32)
            lod[100:160] = rng.choice(_lod_values(L), 60)
            g = rng.standard_normal((n, ct)).astype(np.float32)
            for mode, bias in (('repeat', 0.0), ('clamp', 0.0), ('repeat', 0.25), ('clamp', 0.25)):
                what = '%s ct=%d max_level=%s %s lod_bias=%g' % (shape, ct, max_level, mode, bias)
                r = mr.grad(tex, uv, g, mode, lod=lod, lod_bias=bias, max_level=max_level)
                lam = (lod + np.float32(bias)).astype(np.float32)
                out, (gt, gu, gl) = _spec_grads(tex, uv, g, mode, lam, True, max_level)
                want, mag = mr.sample(tex, uv, mode, lod=lod, lod_bias=bias, max_level=max_level, magnitude=True)
                _close(out, want, mag, what + ' value')
                _close(gt, r['grad_texture'], r['mass_texture'], what + ' grad_texture')
                _close(gu, r['grad_uvs'], r['mass_uvs'], what + ' grad_uvs')
                _close(gl, r['grad_lod'], r['mass_lod'], what + ' grad_lod')


def test_restatement_gradients_with_a_footprint_lod_are_the_spec():
    """The footprint's lambda (mr.footprint_lod, held constant as §7 (5) says) on a masked image."""
    rng = np.random.default_rng(12)
    tex = rng.uniform(-1, 1, (64, 128, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(12.), np.arange(20.), indexing='ij')
    uv = np.stack([np.stack([0.1 + xs * s / 128 + ys * 0.3 / 128, 0.2 + ys * s / 64], -1) for s in (0.5, 3.0, 9.0)]).astype(np.float32)
    mask = (rng.uniform(0, 1, uv.shape[:-1]) > 0.3).astype(np.float32)
    g = rng.standard_normal(uv.shape[:-1] + (3,)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        lam = mr.footprint_lod(uv, 64, 128, mode, mask, -0.2)
        r = mr.grad(tex, uv, g, mode, lod_bias=-0.2, mask=mask)
        _, (gt, gu) = _spec_grads(tex, uv, g, mode, lam, False, None)
        _close(gt, r['grad_texture'], r['mass_texture'], mode + ' grad_texture')
        _close(gu.reshape(uv.shape), r['grad_uvs'], r['mass_uvs'], mode + ' grad_uvs')


def test_restatement_scatters_one_level_where_f_is_zero():
    """§7 (4): where f == 0 only S_l is read and written, so a NaN look-up at an integer lod poisons the 2 x 2 taps of
    level l alone (4 base texels at lod 0; 4 texels of 4 x 4 at lod 2), and at a fractional lod those of l + 1 too."""
    rng = np.random.default_rng(0)
    tex = rng.uniform(-1, 1, (16, 8, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, (3, 2)).astype(np.float32)
    uv[1] = (np.nan, 0.3)
    g = rng.standard_normal((3, 3))
    for lod, rows in ((0.0, 4), (2.0, 64), (2.5, 128)):
        r = mr.grad(tex, uv, g, 'repeat', lod=np.full(3, lod, np.float32))
        assert int(np.isnan(r['grad_texture']).any(-1).sum()) == rows, lod
        assert np.isfinite(r['grad_uvs'][1, 0]) and np.isnan(r['grad_uvs'][1, 1])   # u's weights use v's fraction only
        assert np.isfinite(r['grad_uvs'][[0, 2]]).all()


# ---- the C entry points' argument checks, before any device work (CPU) ------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize('max_level', [None, 0, 1, 2, 5, 40])
def test_mip_levels_entry_point_matches_the_restatement(lib, max_level):
    from dirt_amd import texture as tx
    shapes = [(1, 1), (1, 2), (2, 1), (512, 512), (480, 640), (8, 2), (2, 16), (6, 9), (1, 4096), (4096, 1), (2, 2048),
              (4096, 16), (2048, 2048), (3, 1), (1 << 30, 1), (1, 1 << 30), (1 << 15, 1 << 15), (96, 64), (1000, 8)]
    for (ht, wt) in shapes:
        for ct in (1, 3, 8):
            floats = ctypes.c_longlong(-1)
            levels = lib.dirt_texture_mip_levels(ht, wt, ct, -1 if max_level is None else max_level, ctypes.byref(floats))
            assert levels == mr.level_count(ht, wt, max_level) == len(_spec_dims(ht, wt, max_level)), (ht, wt, max_level)
            assert floats.value == sum(h * w * ct for h, w in _spec_dims(ht, wt, max_level)), (ht, wt, ct, max_level)
            assert lib.dirt_texture_mip_levels(ht, wt, ct, -1 if max_level is None else max_level, None) == levels
            if ht * wt * ct < 1 << 26:
                assert tx._mip_geometry(ht, wt, ct, max_level)[:2] == (levels, floats.value)


def test_mip_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    from dirt_amd import _lib
    E = _lib.E_INVALID_ARGUMENT
    p = ctypes.c_void_p(16)     # never dereferenced: validation fails first
    err = lib.dirt_texture_last_error

    def refused(rc, text):
        assert rc == E, (rc, text)
        assert text.encode() in err(), (text, err())

    for (ht, wt, ct) in ((0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3)):
        refused(lib.dirt_texture_mip_levels(ht, wt, ct, -1, None), 'bad sizes')
        refused(lib.dirt_texture_mip_build(p, p, ht, wt, ct, 1, None), 'bad sizes')
        refused(lib.dirt_texture_mip_collapse(p, p, ht, wt, ct, 1, None), 'bad sizes')
        refused(lib.dirt_texture_sample_mip_forward(p, p, None, None, p, 1, 4, 1, ht, wt, ct, 1, 2, 1, 0.0, 0, None), 'bad sizes')
        refused(lib.dirt_texture_sample_mip_backward(p, p, None, None, p, p, p, p, None, 1, 4, 1, ht, wt, ct, 1, 2, 2, 1, 0.0, 0, None),
                'bad sizes')
    for levels in (0, -1, 5):   # an 8 x 8 texture has 1..4 levels
        refused(lib.dirt_texture_mip_build(p, p, 8, 8, 3, levels, None), 'levels')
        refused(lib.dirt_texture_mip_collapse(p, p, 8, 8, 3, levels, None), 'levels')
        refused(lib.dirt_texture_sample_mip_forward(p, p, None, None, p, 1, 4, 1, 8, 8, 3, levels, 2, 1, 0.0, 0, None), 'levels')
        refused(lib.dirt_texture_sample_mip_backward(p, p, None, None, p, p, p, p, None, 1, 4, 1, 8, 8, 3, levels, 2, 2, 1, 0.0, 0, None),
                'levels')
    refused(lib.dirt_texture_mip_build(None, p, 8, 8, 3, 4, None), 'NULL')
    refused(lib.dirt_texture_mip_build(p, None, 8, 8, 3, 1, None), 'NULL')
    refused(lib.dirt_texture_mip_collapse(None, p, 8, 8, 3, 4, None), 'NULL')
    refused(lib.dirt_texture_mip_collapse(p, None, 8, 8, 3, 1, None), 'NULL')

    def fwd(pyr=p, uvs=p, lod=None, mask=None, out=p, rows=2, cols=4, image_rows=1, levels=4, uv_stride=2, mask_stride=1, flags=0):
        return lib.dirt_texture_sample_mip_forward(pyr, uvs, lod, mask, out, rows, cols, image_rows, 8, 8, 3, levels, uv_stride,
                                                   mask_stride, 0.0, flags, None)

    def bwd(pyr=p, uvs=p, lod=None, mask=None, gout=p, gpyr=p, gtex=p, guv=p, glod=None, rows=2, cols=4, image_rows=1, levels=4,
            uv_stride=2, guv_stride=2, mask_stride=1, flags=0):
        return lib.dirt_texture_sample_mip_backward(pyr, uvs, lod, mask, gout, gpyr, gtex, guv, glod, rows, cols, image_rows, 8, 8, 3,
                                                    levels, uv_stride, guv_stride, mask_stride, 0.0, flags, None)

    for call in (fwd, bwd):
        refused(call(rows=-1), 'bad pixel grid')
        refused(call(cols=-1), 'bad pixel grid')
        refused(call(rows=1 << 32, cols=1 << 32), 'bad pixel grid')
        refused(call(image_rows=0), 'image_rows')
        refused(call(rows=3, image_rows=2), 'image_rows')
        refused(call(uv_stride=1), 'uv_stride < 2')
        refused(call(mask=p, mask_stride=0), 'mask_stride < 1')
        refused(call(pyr=None), 'NULL')
        refused(call(uvs=None), 'NULL')
        refused(call(flags=_lib.TEX_NEAREST), 'DIRT_TEX_NEAREST')
    refused(fwd(out=None), 'out is NULL')
    refused(bwd(gpyr=None), 'NULL')
    refused(bwd(gtex=None), 'NULL')
    refused(bwd(gout=None), 'grad_out is NULL')
    refused(bwd(guv_stride=1), 'grad_uv_stride < 2')
    refused(bwd(glod=p), 'grad_lod needs lod')
    # an empty look-up is a no-op for the forward (no launch): NULL buffers are fine there
    assert fwd(pyr=None, uvs=None, out=None, rows=0) == 0 and err() == b''
    assert fwd(pyr=None, uvs=None, out=None, cols=0, image_rows=1) == 0


# ---- the kernels against the restatement, on the GPU ------------------------------------------------------------------

def _smooth_uv(B, H, W, scale, seed, offset=(0.03, 0.05)):
    """A rotated affine (u, v) field per image: `scale` texture widths across the frame."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = []
    for _ in range(B):
        ang = rng.uniform(-0.4, 0.4)
        c, s = np.cos(ang), np.sin(ang)
        u = (c * xs / W + s * ys / H) * scale + offset[0] + rng.uniform(0, 0.05)
        v = (-s * xs / W + c * ys / H) * scale + offset[1] + rng.uniform(0, 0.05)
        out.append(np.stack([u, v], -1))
    return np.stack(out).astype(np.float32)


LOD_MARGIN = 0.05   # see _lod_margin


def _lod_margin(uv, ht, wt, mode='repeat', mask=None, lod_bias=0.0, max_level=None):
    """The distance of the footprint's lambda from the nearest integer, per pixel (inf where lambda is clamped, not finite,
    or exactly an integer).  The kernels' log2f may differ from numpy's by an ulp, and where lambda lies close to an integer
    one level's weight is tiny: where the other level's term vanishes (index_k clamped at a border, say) that ulp becomes
    a relative error of ulp / distance, which the L1 mass does not cover.  Footprint test data keeps LOD_MARGIN, so no
    footprint test checks the footprint lambda within LOD_MARGIN of a level boundary: lambdas at, just below and around
    integers are covered with an explicit lod (test_texel_and_level_edges), where both sides use the same float32 value."""
    lam = mr.footprint_lod(uv, ht, wt, mode, mask, lod_bias).astype(np.float64)
    top = mr.level_count(ht, wt, max_level) - 1
    with np.errstate(invalid='ignore'):
        d = np.abs(lam - np.rint(lam))
        return np.where(np.isfinite(lam) & (lam > 0) & (lam < top) & (d > 0), d, np.inf)


def _keep_lod_margin(uv, ht, wt, rng, masks=(None,), fixed=None):
    """Redraw the (u, v) of pixels of a random field whose footprint lambda lies within LOD_MARGIN of an integer (in
    either mode, with each mask) -- and of their neighbours -- until none does; `fixed`: pixels left as they are."""
    for _ in range(200):
        bad = np.zeros(uv.shape[:-1], bool)
        for mode in ('repeat', 'clamp'):
            for m in masks:
                bad |= _lod_margin(uv, ht, wt, mode, m) < LOD_MARGIN
        if fixed is not None:
            bad &= ~fixed
        if not bad.any():
            return uv
        uv[bad] = rng.uniform(-0.5, 1.5, (int(bad.sum()), 2)).astype(np.float32)
    raise AssertionError('could not keep the footprint lambda away from integers')


def _lookup(gpu, tex, uv, g, what, mode='repeat', lod=None, lod_bias=0.0, mask=None, max_level=None, t=None, u=None, m=None,
            g_t=None, uv_leaf=None, uv_of=None):
    """Forward and backward of sample_texture_uv(filter='trilinear') against mr.sample / mr.grad.  t, u, m, g_t: the device
    tensors to pass (layouts); uv_leaf: the tensor u is a view of, uv_of(its gradient) -> the gradient of the (u, v) pairs.
    Returns the gradients."""
    from dirt_amd import texture
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True) if t is None else t
    u = torch.from_numpy(uv).to(gpu).requires_grad_(True) if u is None else u
    if m is None and mask is not None:
        m = torch.from_numpy(mask).to(gpu)
    lt = torch.from_numpy(lod).to(gpu).requires_grad_(True) if lod is not None else None
    if lod is None:
        assert _lod_margin(uv, tex.shape[0], tex.shape[1], mode, mask, lod_bias, max_level).min() >= LOD_MARGIN, what + ': test data'
    out = texture.sample_texture_uv(t, u, mode, 'trilinear', lod=lt, lod_bias=lod_bias, mask=m, max_level=max_level)
    want, mag = mr.sample(tex, uv, mode, lod=lod, lod_bias=lod_bias, mask=mask, max_level=max_level, magnitude=True)
    _close(out, want, mag, what + ' forward')
    leaves = [t, u if uv_leaf is None else uv_leaf] + ([lt] if lt is not None else [])
    grads = torch.autograd.grad(out, leaves, torch.from_numpy(g).to(gpu) if g_t is None else g_t)
    r = mr.grad(tex, uv, g, mode, lod=lod, lod_bias=lod_bias, mask=mask, max_level=max_level)
    _close(grads[0], r['grad_texture'], r['mass_texture'], what + ' grad_texture')
    guv = grads[1] if uv_of is None else uv_of(grads[1])
    _close(guv, r['grad_uvs'], r['mass_uvs'], what + ' grad_uvs')
    if lt is not None:
        _close(grads[2], r['grad_lod'], r['mass_lod'], what + ' grad_lod')
    return grads


def _bits_equal(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), '%s: %d elements differ' % (what, int(np.sum(got != want)))


def _pool_pyramid_grad(t, gs):
    """dL/dtexture of sum_k <level_k, g_k> through torch's avg_pool2d composition."""
    t2 = t.detach().clone().requires_grad_(True)
    lv, loss = t2, (t2 * gs[0]).sum()
    for g in gs[1:]:
        kh, kw = (2 if lv.shape[0] > 1 else 1), (2 if lv.shape[1] > 1 else 1)
        lv = torch.nn.functional.avg_pool2d(lv.permute(2, 0, 1)[None], (kh, kw))[0].permute(1, 2, 0)
        loss = loss + (lv * g).sum()
    loss.backward()
    return t2.grad


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2048, 2048, 3), (4096, 16, 3), (1, 4096, 3), (4096, 1, 3), (2, 2048, 3), (256, 192, 2),
                                   (128, 160, 8)])
def test_pyramid_bit_exact_and_backward_at_every_split(gpu, shape):
    """2048² x 3: level 6 has 3 072 floats, so the top kernel's 1 024 threads stride; 12.6 M texture floats, past the
    collapse's grid cap of 4 194 304.  Thin textures (2 x 1 means), and Ct = 2 and 8 (channel passes of four) over many
    32 x 32 blocks."""
    from dirt_amd import texture
    rng = np.random.default_rng(sum(shape))
    tex = rng.uniform(-1, 1, shape).astype(np.float32)
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    got = texture.mip_pyramid(t)
    want = mr.pyramid(tex)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        _bits_equal(a, b, 'level %d of %s' % (k, shape))
    gen = torch.Generator(device=gpu).manual_seed(7)
    gs = [torch.randn(tuple(lv.shape), device=gpu, generator=gen) for lv in got]
    sum((lv * g).sum() for lv, g in zip(got, gs)).backward()
    assert torch.allclose(t.grad, _pool_pyramid_grad(t, gs), rtol=1e-5, atol=1e-5), shape


@pytest.mark.gpu
def test_pyramid_at_every_max_level(gpu):
    """max_level 0 (a copy, and a collapse with one level) up to the natural count + 2 on one texture: below 5 the block
    kernel reduces fewer levels (kt) in smaller blocks."""
    from dirt_amd import texture
    rng = np.random.default_rng(3)
    tex = rng.uniform(-1, 1, (128, 256, 3)).astype(np.float32)
    natural = mr.level_count(128, 256)
    assert natural == 9
    for max_level in range(0, natural + 3):
        t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
        got = texture.mip_pyramid(t, max_level=max_level)
        want = mr.pyramid(tex, max_level)
        assert len(got) == len(want) == min(max_level + 1, natural)
        for k, (a, b) in enumerate(zip(got, want)):
            _bits_equal(a, b, 'level %d, max_level %d' % (k, max_level))
        gs = [torch.from_numpy(rng.standard_normal(tuple(lv.shape)).astype(np.float32)).to(gpu) for lv in got]
        sum((lv * g).sum() for lv, g in zip(got, gs)).backward()
        assert torch.allclose(t.grad, _pool_pyramid_grad(t, gs), rtol=1e-5, atol=1e-5), max_level


_SPECIALS = [(np.nan, 0.3), (0.3, np.nan), (np.nan, np.nan), (np.inf, 0.4), (-np.inf, 0.4), (0.4, np.inf), (0.4, -np.inf),
             (np.inf, -np.inf), (np.nan, np.inf)]


def _near_origin_uv(B, H, W, ht, wt):
    """Images whose first 16 x 16 tile lies at the texture's top-left corner, 1.4 texels per pixel (lambda about 0.5): the
    taps of a coordinate whose index is 0 (NaN, or +-inf in repeat mode) stay inside that tile's LDS patches."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    uv = np.stack([(0.3 + 1.4 * xs + 0.2 * ys) / wt, (0.4 + 1.4 * ys + 0.1 * xs) / ht], -1)
    return np.broadcast_to(uv, (B, H, W, 2)).astype(np.float32)


def _put(uv, at, pair):
    """uv[at] = pair, keeping the field's value where the pair holds None."""
    uv[at] = [x if y is None else y for x, y in zip(uv[at], pair)]


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_non_finite_input(gpu, ct):
    """NaN and +-inf in u and / or v, with the footprint lod (and a mask) and with an explicit lod; NaN and +-inf in lod; a
    NaN lod_bias.  Images: 0 a smooth field, 1 a random one (fallback tiles), 2 and 3 fields at the texture's corner whose
    first tile holds NaN (2) and +-inf (3) coordinates and takes the LDS patch path -- asserted with the kernel's rule --
    so NaN sums in the patch and its flush are checked.  The forward and the gradients are non-finite exactly where the
    restatement's are and within tolerance elsewhere.  A NaN coordinate makes its own footprint lambda NaN (-> 0) and
    its neighbours' differences NaN: fmax takes the other axis, and a pixel whose two forward neighbours are NaN gets NaN
    (-> 0) too."""
    rng = np.random.default_rng(50 + ct)
    Ht, Wt, H, W = 64, 128, 32, 48
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = np.concatenate([_smooth_uv(1, H, W, 2.6, ct), rng.uniform(-0.5, 1.5, (1, H, W, 2)).astype(np.float32),
                         _near_origin_uv(2, H, W, Ht, Wt)])
    nan, inf = np.nan, np.inf
    special = np.zeros(uv.shape[:-1], bool)
    for b in range(2):
        for k, sp in enumerate(_SPECIALS):
            special[b, 5 + 3 * k, 7 + 4 * k] = True
            _put(uv, (b, 5 + 3 * k, 7 + 4 * k), sp)
    for b, r, c in ((0, 0, 20), (1, 0, 20), (2, 5, 9)):   # NaN at both forward neighbours of (r, c): its lambda is NaN
        for at in ((b, r, c + 1), (b, r + 1, c)):
            special[at] = True
            _put(uv, at, (nan, nan))
    for at, sp in (((2, 3, 5), (nan, None)), ((2, 7, 2), (None, nan)), ((2, 11, 12), (nan, nan)), ((2, 14, 4), (nan, None)),
                   ((3, 2, 3), (inf, None)), ((3, 4, 11), (-inf, None)), ((3, 8, 6), (None, inf)), ((3, 12, 13), (None, -inf)),
                   ((3, 13, 2), (inf, -inf)), ((3, 10, 9), (nan, inf))):
        special[at] = True
        _put(uv, at, sp)
    mask = (rng.uniform(0, 1, uv.shape[:-1]) > 0.2).astype(np.float32)
    _keep_lod_margin(uv[1:2], Ht, Wt, rng, (None, mask[1:2]), special[1:2])
    with np.errstate(invalid='ignore'):
        for mode in ('repeat', 'clamp'):
            lam = mr.footprint_lod(uv, Ht, Wt, mode)
            for b, r, c in ((0, 0, 20), (1, 0, 20), (2, 5, 9)):
                assert np.isfinite(uv[b, r, c]).all() and np.isnan(lam[b, r, c]), (mode, b, r, c)
            for m in (None, mask):
                tiles = _tile_patch_texels(uv, Ht, Wt, mode, mask=m)
                assert 0 < tiles[2 * H // 16, 0] <= 1600, (mode, m is None, tiles[2 * H // 16, 0])        # NaN (image 2)
                if mode == 'repeat':                                                                   # +-inf -> index NaN
                    assert 0 < tiles[3 * H // 16, 0] <= 1600, (mode, m is None, tiles[3 * H // 16, 0])
    g = rng.standard_normal(uv.shape[:-1] + (ct,)).astype(np.float32)
    lod = rng.uniform(-0.5, 6.5, uv.shape[:-1]).astype(np.float32)
    lod[:, 3, :6] = [np.nan, np.inf, -np.inf, np.nan, 2.0, 3.5]
    lod[:, 5 + 3 * 0, 7] = 2.5                     # a NaN coordinate at a fractional lod: both levels poisoned
    for mode in ('repeat', 'clamp'):
        what = 'ct=%d %s' % (ct, mode)
        _lookup(gpu, tex, uv, g, what + ' footprint', mode)
        _lookup(gpu, tex, uv, g, what + ' footprint+mask', mode, mask=mask)
        _lookup(gpu, tex, uv, g, what + ' lod', mode, lod=lod)
        _lookup(gpu, tex, uv, g, what + ' NaN lod_bias', mode, lod=lod, lod_bias=float('nan'))
        _lookup(gpu, tex, uv, g, what + ' footprint, NaN lod_bias', mode, lod_bias=float('nan'))


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_texel_and_level_edges(gpu, ct):
    """(u, v) on level-0 and coarser texel edges, within half a coarse texel of the top / left border (index_k clamps to
    0 and its derivative 1/s drops to 0), 0, -0.0, 1, 1 - 2^-24 and whole numbers; lambda at every integer, one float32
    step below it, at L - 1 and beyond.  As images (16 x 16 tiles) and as a flat list."""
    rng = np.random.default_rng(70 + ct)
    Ht, Wt = 32, 64
    L = mr.level_count(Ht, Wt)
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    us, vs = np.asarray(_edge_values(Wt), np.float32), np.asarray(_edge_values(Ht), np.float32)
    grid = np.stack(np.meshgrid(us, vs), -1).astype(np.float32)              # [len(vs), len(us), 2]
    lods = np.asarray(_lod_values(L), np.float32)
    uv = np.broadcast_to(grid, (len(lods),) + grid.shape).copy()
    lod = np.broadcast_to(lods[:, None, None], uv.shape[:-1]).copy()
    g = rng.standard_normal(uv.shape[:-1] + (ct,)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        _lookup(gpu, tex, uv, g, 'edges ct=%d %s' % (ct, mode), mode, lod=lod)
        _lookup(gpu, tex, uv.reshape(-1, 2), g.reshape(-1, ct), 'edges flat ct=%d %s' % (ct, mode), mode, lod=lod.reshape(-1))
    _lookup(gpu, tex, grid[None], g[:1], 'edges footprint ct=%d' % ct, 'clamp', lod_bias=0.25)


@pytest.mark.gpu
def test_layouts(gpu):
    """Ct = 4 with the texture and grad_out one float into their buffers (the generic backward kernel); (u, v) read in
    place from channels 2:4 of a 7-channel G-buffer with its mask at channel 0 (strides 7); uvs [A, B, H, W, 2]; images
    [1, W, 2], [H, 1, 2], [B, 1, 1, 2]; empty look-ups."""
    from dirt_amd import texture
    rng = np.random.default_rng(90)
    tex4 = rng.uniform(-1, 1, (64, 32, 4)).astype(np.float32)
    uv = _smooth_uv(2, 24, 40, 2.5, 1)
    g = rng.standard_normal((2, 24, 40, 4)).astype(np.float32)
    tbuf = torch.zeros(tex4.size + 1, device=gpu)
    tbuf[1:] = torch.from_numpy(tex4.reshape(-1)).to(gpu)
    t = tbuf[1:].view(tex4.shape).requires_grad_(True)
    gbuf = torch.zeros(g.size + 1, device=gpu)
    gbuf[1:] = torch.from_numpy(g.reshape(-1)).to(gpu)
    g_t = gbuf[1:].view(g.shape)
    assert t.data_ptr() % 16 and g_t.data_ptr() % 16
    for mode in ('repeat', 'clamp'):
        _lookup(gpu, tex4, uv, g, 'misaligned ct=4 %s' % mode, mode, t=t, g_t=g_t)
        _lookup(gpu, tex4, uv, g, 'misaligned ct=4 lod %s' % mode, mode, lod=rng.uniform(-1, 6, uv.shape[:-1]).astype(np.float32),
                t=t, g_t=g_t)

    tex = rng.uniform(-1, 1, (128, 64, 3)).astype(np.float32)
    gb = np.zeros((2, 24, 40, 7), np.float32)
    gb[..., 2:4] = _smooth_uv(2, 24, 40, 4.0, 2)
    gb[..., 0] = (rng.uniform(0, 1, (2, 24, 40)) > 0.3).astype(np.float32)
    gb[..., 1], gb[..., 4:] = 5.0, 7.0
    gb_t = torch.from_numpy(gb).to(gpu).requires_grad_(True)
    g3 = rng.standard_normal((2, 24, 40, 3)).astype(np.float32)
    grads = _lookup(gpu, tex, gb[..., 2:4], g3, 'gbuffer', 'clamp', mask=gb[..., 0], u=gb_t[..., 2:4], m=gb_t[..., 0],
                    uv_leaf=gb_t, uv_of=lambda x: x[..., 2:4])
    assert not grads[1][..., :2].any() and not grads[1][..., 4:].any()

    uv5 = _smooth_uv(6, 10, 12, 3.0, 3).reshape(2, 3, 10, 12, 2)
    _lookup(gpu, tex, uv5, rng.standard_normal((2, 3, 10, 12, 3)).astype(np.float32), '[A, B, H, W, 2]')
    for shape in ((1, 300, 2), (300, 1, 2), (4, 1, 1, 2), (1, 1, 2)):
        uvs = rng.uniform(-0.2, 1.2, shape).astype(np.float32)
        if shape == (1, 300, 2):
            uvs = _smooth_uv(1, 1, 300, 6.0, 4)[0]
        elif shape == (300, 1, 2):
            uvs = _smooth_uv(1, 300, 1, 6.0, 5)[0]
        gg = rng.standard_normal(shape[:-1] + (3,)).astype(np.float32)
        for mode in ('repeat', 'clamp'):
            _lookup(gpu, tex, uvs, gg, 'image %s %s' % (shape, mode), mode)
            _lookup(gpu, tex, uvs, gg, 'image %s %s lod' % (shape, mode), mode, lod=rng.uniform(-1, 8, shape[:-1]).astype(np.float32))

    for shape, with_lod in (((0, 2), True), ((2, 0, 5, 2), False), ((2, 3, 0, 2), True)):
        t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
        u = torch.zeros(shape, device=gpu, requires_grad=True)
        lod = torch.zeros(shape[:-1], device=gpu, requires_grad=True) if with_lod else None
        out = texture.sample_texture_uv(t, u, 'repeat', 'trilinear', lod=lod)
        assert tuple(out.shape) == shape[:-1] + (3,)
        gt, gu = torch.autograd.grad(out, [t, u], torch.zeros_like(out))
        assert gu.shape == u.shape and torch.equal(gt, torch.zeros_like(gt)), shape


@pytest.mark.gpu
def test_forward_past_the_grid_cap(gpu):
    """2 x 1 025 x 2 048 = 4 198 400 look-ups, past the forward's grid of 16 384 x 256 = 4 194 304 lanes: the grid stride."""
    from dirt_amd import texture
    rng = np.random.default_rng(11)
    tex = rng.uniform(-1, 1, (64, 32, 1)).astype(np.float32)
    uv = rng.uniform(-0.2, 1.2, (2, 1025, 2048, 2)).astype(np.float32)
    lod = rng.uniform(-0.5, 6.5, (2, 1025, 2048)).astype(np.float32)
    out = texture.sample_texture_uv(torch.from_numpy(tex).to(gpu), torch.from_numpy(uv).to(gpu), 'repeat', 'trilinear',
                                    lod=torch.from_numpy(lod).to(gpu))
    want, mag = mr.sample(tex, uv, 'repeat', lod=lod, magnitude=True)
    _close(out, want, mag, 'forward past the grid cap')


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [2.3, 4.6])
def test_minified_gradients_from_a_large_texture(gpu, scale):
    """A 2048² x 3 texture seen at about 2x and 4x minification (footprint lod, lambda about 1.2 and 2.2; see
    _lod_margin): every value and gradient checked."""
    rng = np.random.default_rng(int(20 + 10 * scale))
    tex = rng.uniform(-1, 1, (2048, 2048, 3)).astype(np.float32)
    H, W = (256, 320) if scale < 4 else (192, 256)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    a = 0.1
    u = (np.cos(a) * xs + np.sin(a) * ys) * scale / 2048 + 0.013
    v = (-np.sin(a) * xs + np.cos(a) * ys) * scale / 2048 + 0.21
    uv = np.stack([u, v], -1)[None].astype(np.float32)
    g = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    _lookup(gpu, tex, uv, g, 'minified %gx' % scale)


def _tile_patch_texels(uv, ht, wt, mode='repeat', lod=None, lod_bias=0.0, mask=None):
    """The backward kernel's choice per 16 x 16 tile of the look-up grid of images uv [..., H, W, 2] (H > 1): the texels of
    the tile's LDS patches -- the bounding boxes of its taps at the (at most two adjacent) levels it touches, each counted
    up to 1 601 -- or -1 where its levels span more than two.  The tile takes the patch path iff 0 < value <= 1 600."""
    W = uv.shape[-2]
    rows = int(np.prod(uv.shape[:-2]))
    pyr = [np.zeros((h, w, 1), np.float32) for h, w in _spec_dims(ht, wt, None)]
    L = len(pyr)
    lam = mr._lambda(uv, ht, wt, mode, lod, lod_bias, mask).reshape(-1)
    idx = mr._indices(uv.reshape(-1, 2), ht, wt, mode, np.float32)
    lev, f = mr._split(lam, L, np.float32)
    two = f != 0
    sets = ((mr._Look(pyr, lev, idx[:, 0], idx[:, 1], np.float32), lev, np.ones(len(lev), bool)),
            (mr._Look(pyr, np.minimum(lev + 1, L - 1), idx[:, 0], idx[:, 1], np.float32), np.minimum(lev + 1, L - 1), two))
    out = np.zeros(((rows + 15) // 16, (W + 15) // 16), np.int64)
    pix = np.arange(rows * W).reshape(rows, W)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            sel = pix[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].reshape(-1)
            lmin, lmax = lev[sel].min(), np.where(two[sel], lev[sel] + 1, lev[sel]).max()
            if lmax - lmin > 1:
                out[ty, tx] = -1
                continue
            used = 0
            for level in (lmin, lmin + 1):
                r0, r1, c0, c1 = [], [], [], []
                for look, lv, on in sets:
                    m = sel[on[sel] & (lv[sel] == level)]
                    r0.append(look.r0[m]); r1.append(look.r1[m]); c0.append(look.c0[m]); c1.append(look.c1[m])
                r0, r1, c0, c1 = (np.concatenate(x) for x in (r0, r1, c0, c1))
                if r0.size:
                    used += min(int((r1.max() - r0.min() + 1) * (c1.max() - c0.min() + 1)), 1601)
            out[ty, tx] = used
    return out


@pytest.mark.gpu
def test_patch_of_exactly_1600_texels_and_one_more(gpu):
    """One 16 x 16 tile over a 256 x 256 texture at the constant lod 0.5 (levels 0 and 1), (u, v) affine in the pixel:
    column index 10.25 + 1.75 x, row index 20.25 + 2.8125 y gives taps in boxes of 44 x 28 texels (level 0) and 23 x 16
    (level 1) = 1 600, which the LDS patch holds; column 10 + 3.25 x, row 20.5 + 1.5 y gives 25 x 50 + 13 x 27 = 1 601,
    which falls back to global atomics.  Both paths agree with the restatement at the same tolerance."""
    rng = np.random.default_rng(16)
    ht = wt = 256
    tex = rng.uniform(-1, 1, (ht, wt, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(16.), np.arange(16.), indexing='ij')
    lod = np.full((1, 16, 16), 0.5, np.float32)
    g = rng.standard_normal((1, 16, 16, 3)).astype(np.float32)
    for (c0, sx, r0, sy), texels in (((10.25, 1.75, 20.25, 2.8125), 1600), ((10.0, 3.25, 20.5, 1.5), 1601)):
        uv = np.stack([(c0 + xs * sx) / wt, (r0 + ys * sy) / ht], -1)[None].astype(np.float32)
        assert _tile_patch_texels(uv, ht, wt, lod=lod).tolist() == [[texels]]
        for mode in ('repeat', 'clamp'):
            _lookup(gpu, tex, uv, g, 'patch of %d texels %s' % (texels, mode), mode, lod=lod)


@pytest.mark.gpu
def test_entry_points_with_what_python_never_passes(gpu):
    """Through ctypes: image_rows smaller than the rows given (stacked images), grad_uv_stride = 5, `levels` below the
    natural count on a full pyramid, and a NULL grad_uvs -- against the restatement."""
    from dirt_amd import _lib, rasterise_ops as ops
    lib = _lib.load()
    stream = ops._stream_handle(gpu)
    rng = np.random.default_rng(33)
    Ht, Wt, ct = 64, 128, 3
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    full = mr.level_count(Ht, Wt)
    floats = ctypes.c_longlong(0)
    assert lib.dirt_texture_mip_levels(Ht, Wt, ct, -1, ctypes.byref(floats)) == full
    t = torch.from_numpy(tex).to(gpu)
    pyr = torch.empty(floats.value, device=gpu)
    assert lib.dirt_texture_mip_build(t.data_ptr(), pyr.data_ptr(), Ht, Wt, ct, full, stream) == 0
    scratch = torch.empty(floats.value, device=gpu)

    # a 32 x 40 image passed as two stacked 16-row images: the footprint never crosses row 15 / 16
    uv = _smooth_uv(1, 32, 40, 3.0, 8)[0]
    stacked = uv.reshape(2, 16, 40, 2)
    u = torch.from_numpy(uv).to(gpu)
    out = torch.empty(32 * 40 * ct, device=gpu)
    for flags, mode in ((0, 'repeat'), (_lib.TEX_CLAMP, 'clamp')):
        assert lib.dirt_texture_sample_mip_forward(pyr.data_ptr(), u.data_ptr(), None, None, out.data_ptr(), 32, 40, 16, Ht, Wt, ct,
                                                   full, 2, 1, 0.0, flags, stream) == 0
        want, mag = mr.sample(tex, stacked, mode, magnitude=True)
        _close(out.view(2, 16, 40, ct), want, mag, 'image_rows=16 %s forward' % mode)
        g = rng.standard_normal((2, 16, 40, ct)).astype(np.float32)
        g_t = torch.from_numpy(g).to(gpu)
        gtex = torch.empty_like(t)
        guv = torch.full((32 * 40, 5), 123.0, device=gpu)
        assert lib.dirt_texture_sample_mip_backward(pyr.data_ptr(), u.data_ptr(), None, None, g_t.data_ptr(), scratch.data_ptr(),
                                                    gtex.data_ptr(), guv.data_ptr(), None, 32, 40, 16, Ht, Wt, ct, full, 2, 5, 1, 0.0,
                                                    flags, stream) == 0
        r = mr.grad(tex, stacked, g, mode)
        _close(gtex, r['grad_texture'], r['mass_texture'], 'image_rows=16 %s grad_texture' % mode)
        _close(guv[:, :2].reshape(2, 16, 40, 2), r['grad_uvs'], r['mass_uvs'], 'grad_uv_stride=5 %s grad_uvs' % mode)
        assert torch.all(guv[:, 2:] == 123.0), 'grad_uv_stride=5 wrote between the pairs'

    # three levels of the full pyramid, explicit lod; the backward without grad_uvs
    flat = rng.uniform(-0.2, 1.2, (700, 2)).astype(np.float32)
    lod = rng.uniform(-1, 5, 700).astype(np.float32)
    f_t, l_t = torch.from_numpy(flat).to(gpu), torch.from_numpy(lod).to(gpu)
    out = torch.empty(700 * ct, device=gpu)
    assert lib.dirt_texture_sample_mip_forward(pyr.data_ptr(), f_t.data_ptr(), l_t.data_ptr(), None, out.data_ptr(), 1, 700, 1, Ht, Wt,
                                               ct, 3, 2, 1, 0.5, 0, stream) == 0
    want, mag = mr.sample(tex, flat, lod=lod, lod_bias=0.5, max_level=2, magnitude=True)
    _close(out.view(700, ct), want, mag, 'levels=3 forward')
    g = rng.standard_normal((700, ct)).astype(np.float32)
    g_t = torch.from_numpy(g).to(gpu)
    gtex, glod = torch.empty_like(t), torch.empty(700, device=gpu)
    assert lib.dirt_texture_sample_mip_backward(pyr.data_ptr(), f_t.data_ptr(), l_t.data_ptr(), None, g_t.data_ptr(), scratch.data_ptr(),
                                                gtex.data_ptr(), None, glod.data_ptr(), 1, 700, 1, Ht, Wt, ct, 3, 2, 2, 1, 0.5, 0,
                                                stream) == 0
    r = mr.grad(tex, flat, g, lod=lod, lod_bias=0.5, max_level=2)
    _close(gtex, r['grad_texture'], r['mass_texture'], 'levels=3, NULL grad_uvs: grad_texture')
    _close(glod, r['grad_lod'], r['mass_lod'], 'levels=3, NULL grad_uvs: grad_lod')


@pytest.mark.gpu
def test_deferred_trilinear_shader_matches_manual_composition(gpu, oracle):
    """rasterise_deferred with a shader that samples a texture trilinearly at the G-buffer's (u, v) (channels 1:3), the
    footprint's neighbours masked by gbuffer[..., 0]: pixels = shader(the oracle's G-buffer); grad_texture is mr.grad's
    on that G-buffer; the vertex and attribute gradients are the oracle's for the shaded image and the G-buffer gradient."""
    from tests import parity, scenes
    from dirt_amd import rasterise_ops as ops, texture
    s = scenes.rand_scene(200, 48, 64, 4, 23, 0.05, 0.3)
    rng = np.random.default_rng(23)
    V = s['vertices'].shape[0]
    s['vertex_colors'][:, 0] = 1.0                                   # the mask: 1 on every face, 0 on the background
    s['vertex_colors'][:, 1:3] = rng.uniform(-0.2, 1.2, (V, 2))       # (u, v)
    s['background'][:] = 0.0
    tex = rng.uniform(0, 1, (128, 256, 3)).astype(np.float32)
    bg = torch.from_numpy(s['background']).to(gpu).requires_grad_(True)
    v = torch.from_numpy(s['vertices']).to(gpu).requires_grad_(True)
    attrs = torch.from_numpy(s['vertex_colors']).to(gpu).requires_grad_(True)
    f = torch.from_numpy(s['faces']).to(gpu)
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)

    def shader(gbuffer, texture_):
        unlit = texture.sample_texture_uv(texture_, gbuffer[..., 1:3], 'repeat', 'trilinear', mask=gbuffer[..., 0])
        return unlit * gbuffer[..., 3:4] * gbuffer[..., :1]

    px = ops.rasterise_deferred(bg, v, attrs, f, shader, [t])
    d = rng.standard_normal((48, 64, 3)).astype(np.float32)
    px.backward(torch.from_numpy(d).to(gpu))

    gbuf = oracle.forward(s['background'][None], s['vertices'][None], s['vertex_colors'][None], s['faces'][None])
    gt = torch.from_numpy(gbuf[0]).to(gpu).requires_grad_(True)
    t2 = t.detach().clone().requires_grad_(True)
    shaded = shader(gt, t2)
    assert torch.allclose(px, shaded.detach(), atol=1e-6)
    unlit = texture.sample_texture_uv(t2.detach(), gt.detach()[..., 1:3], 'repeat', 'trilinear', mask=gt.detach()[..., 0])
    want, mag = mr.sample(tex, gbuf[0, ..., 1:3], 'repeat', mask=gbuf[0, ..., 0], magnitude=True)
    _close(unlit, want, mag, 'deferred forward')
    shaded.backward(torch.from_numpy(d).to(gpu))
    g_unlit = d * gbuf[0, ..., 3:4] * gbuf[0, ..., :1]
    r = mr.grad(tex, gbuf[0, ..., 1:3], g_unlit, 'repeat', mask=gbuf[0, ..., 0])
    _close(t.grad, r['grad_texture'], r['mass_texture'], 'deferred grad_texture')
    _close(t2.grad, r['grad_texture'], r['mass_texture'], 'composed grad_texture')
    want_v = oracle.backward(s['vertices'][None], s['faces'][None], shaded.detach().cpu().numpy()[None], d[None])
    want_a = oracle.backward(s['vertices'][None], s['faces'][None], gbuf, gt.grad.cpu().numpy()[None])
    parity.grad_close(v.grad, want_v, 'grad_vertices', 'vertices', 0)
    parity.grad_close(attrs.grad, want_a, 'grad_vertex_colors', 'attributes', 0)
    assert np.array_equal(bg.grad.cpu().numpy(), want_a['grad_background'][0]), 'background'
