"""The fused texture look-up (dirt_amd.texture.sample_texture_uv; include/dirt_hip.h dirt_texture_sample_*) against the
numpy restatement of the reference's samples/textured.py:16-61 (oracle/texture_oracle.py) and against the composed torch
helpers; the oracle itself against analytic cases on the CPU."""
import numpy as np
import pytest
import torch

from oracle import texture_oracle as tex_oracle


def test_oracle_texel_centres_and_ramps():
    """Sampling at integer indices returns the texel; a texture linear in (row, column) is reproduced exactly between
    texels (no half-texel shift: the reference blends by the fraction of the index)."""
    rng = np.random.default_rng(0)
    ht, wt = 6, 9
    tex = rng.uniform(0, 1, (ht, wt, 3)).astype(np.float32)
    rows, cols = np.meshgrid(np.arange(ht), np.arange(wt), indexing='ij')
    uv = np.stack([cols / wt, rows / ht], -1).astype(np.float32)          # (u, v) = (column, row) / size, top-left origin
    got = tex_oracle.sample_texture_uv(tex, uv)
    assert np.allclose(got, tex, atol=1e-6)
    ramp = (2.0 * rows + 0.5 * cols)[..., None].astype(np.float32) * np.ones(3, np.float32)
    uvf = np.stack([(cols[:-1, :-1] + 0.25) / wt, (rows[:-1, :-1] + 0.75) / ht], -1).astype(np.float32)
    got = tex_oracle.sample_texture_uv(ramp, uvf)
    want = (2.0 * (rows[:-1, :-1] + 0.75) + 0.5 * (cols[:-1, :-1] + 0.25))[..., None] * np.ones(3)
    assert np.allclose(got, want, atol=1e-4)
    # repeat wraps, clamp saturates
    assert np.allclose(tex_oracle.sample_texture_uv(tex, uv + 3.0), tex_oracle.sample_texture_uv(tex, uv), atol=1e-5)
    edge = tex_oracle.sample_texture_uv(tex, np.array([[5.0, -2.0]], np.float32), mode='clamp')
    assert np.allclose(edge[0], tex[0, wt - 1])


def test_oracle_gradient_is_the_finite_difference():
    rng = np.random.default_rng(1)
    tex = rng.uniform(0, 1, (5, 7, 2)).astype(np.float32)
    uv = rng.uniform(0.05, 0.8, (11, 2)).astype(np.float32)
    g = rng.standard_normal((11, 2)).astype(np.float32)
    gt, guv = tex_oracle.sample_texture_uv_grad(tex, uv, g)
    eps = 1e-3
    for i in range(3):
        for k in range(2):
            up, dn = uv.copy(), uv.copy()
            up[i, k] += eps; dn[i, k] -= eps
            fd = ((tex_oracle.sample_texture_uv(tex, up).astype(np.float64) - tex_oracle.sample_texture_uv(tex, dn)) * g).sum() / (2 * eps)
            assert abs(fd - guv[i, k]) <= 2e-2 * max(1.0, abs(fd)), (i, k, fd, guv[i, k])
    t2 = tex.copy(); t2[2, 3, 1] += 0.5
    fd = ((tex_oracle.sample_texture_uv(t2, uv).astype(np.float64) - tex_oracle.sample_texture_uv(tex, uv)) * g).sum() / 0.5
    assert abs(fd - gt[2, 3, 1]) <= 1e-4 * max(1.0, abs(fd))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
@pytest.mark.parametrize('filt', ['bilinear', 'nearest'])
def test_fused_lookup_matches_oracle_and_composition(gpu, mode, filt):
    from dirt_amd import texture
    rng = np.random.default_rng(3)
    tex = rng.uniform(0, 1, (37, 53, 3)).astype(np.float32)
    uv = rng.uniform(-1.5, 2.5, (48, 64, 2)).astype(np.float32)
    uv[0, :8] = [[0.0, 0.0], [1.0, 1.0], [0.999999, 0.5], [-1e-9, 0.3], [0.5, -1e-9], [1.0, 0.0], [0.0, 1.0], [2.0, -3.0]]
    want = tex_oracle.sample_texture_uv(tex, uv, mode, filt)
    t, u = torch.from_numpy(tex).to(gpu), torch.from_numpy(uv).to(gpu)
    got = texture.sample_texture_uv(t, u, mode, filt)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), 'differs from the oracle'
    composed = texture.sample_texture(t, texture.uvs_to_pixel_indices(u, t.shape[:2], mode), filt)
    assert torch.equal(got, composed), 'differs from the composed torch helpers'


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
def test_fused_lookup_gradients_in_place_from_a_gbuffer(gpu, mode):
    """(u, v) read in place from channels 1:3 of a 6-channel G-buffer (samples/textured.py:120-122), gradients against the
    oracle and against autograd through the composed helpers."""
    from dirt_amd import texture
    rng = np.random.default_rng(4)
    tex = rng.uniform(0, 1, (20, 31, 3)).astype(np.float32)
    gbuf = rng.uniform(-0.4, 1.4, (40, 56, 6)).astype(np.float32)
    g = rng.standard_normal((40, 56, 3)).astype(np.float32)
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    gb = torch.from_numpy(gbuf).to(gpu).requires_grad_(True)
    out = texture.sample_texture_uv(t, gb[..., 1:3], mode)
    out.backward(torch.from_numpy(g).to(gpu))
    want_t, want_uv = tex_oracle.sample_texture_uv_grad(tex, gbuf[..., 1:3], g, mode)
    assert float(np.abs(t.grad.cpu().numpy() - want_t).max()) <= 1e-4 * max(1.0, float(np.abs(want_t).max()))
    got_uv = gb.grad.cpu().numpy()
    assert float(np.abs(got_uv[..., 1:3] - want_uv).max()) <= 1e-4 * max(1.0, float(np.abs(want_uv).max()))
    assert not got_uv[..., 0].any() and not got_uv[..., 3:].any()
    _, _, mass_t, mass_uv = tex_oracle.sample_texture_uv_grad(tex, gbuf[..., 1:3], g, mode, want_mass=True)
    _per_element(t.grad, want_t, mass_t, 'grad_texture')
    _per_element(got_uv[..., 1:3], want_uv, mass_uv, 'grad_uvs')
    t2 = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    gb2 = torch.from_numpy(gbuf).to(gpu).requires_grad_(True)
    texture.sample_texture(t2, texture.uvs_to_pixel_indices(gb2[..., 1:3], t2.shape[:2], mode)).backward(torch.from_numpy(g).to(gpu))
    assert torch.allclose(t.grad, t2.grad, atol=1e-4, rtol=1e-4)
    assert torch.allclose(gb.grad, gb2.grad, atol=1e-3, rtol=1e-4)


def test_argument_shapes_are_checked():
    """`[..., 3]` coordinates or a 2-D texture are refused instead of being read as the wrong pairs (no GPU needed: the
    checks come before any device work)."""
    from dirt_amd import texture as tex
    with pytest.raises(ValueError):
        tex.sample_texture_uv(torch.zeros(4, 4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError):
        tex.sample_texture_uv(torch.zeros(4, 4), torch.zeros(5, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
def test_gradient_of_a_smooth_uv_image_takes_the_patch_path(gpu, ct, mode):
    """The backward kernel works on 16 x 16-pixel tiles of the look-up image and sums each tile's contributions in an LDS copy of
    the texture patch they fall into (dirt_texture.hip, round 6); tiles whose patch is too large -- the `repeat` seam of this
    field, random coordinates -- scatter float atomics as before.  A smooth, rotated (u, v) field with a seam across the
    frame exercises both, for every channel-count specialisation (1, 3, 4; 5 = the generic passes), an odd image size and a
    batch of two images; values against the oracle's float64 gradient."""
    from dirt_amd import texture
    rng = np.random.default_rng(11 + ct)
    H, W, Ht, Wt = 75, 93, 64, 48
    tex = rng.uniform(0, 1, (Ht, Wt, ct)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    uvs = []
    for b, (ang, scale) in enumerate(((0.3, 1.7), (-0.2, 0.6))):
        c, s = np.cos(ang), np.sin(ang)
        u = (c * xs / W + s * ys / H) * scale - 0.2
        v = (-s * xs / W + c * ys / H) * scale + 0.1
        uvs.append(np.stack([u, v], -1))
    uv = np.stack(uvs).astype(np.float32)                     # [2, H, W, 2]
    g = rng.standard_normal((2, H, W, ct)).astype(np.float32)
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    u_t = torch.from_numpy(uv).to(gpu).requires_grad_(True)
    out = texture.sample_texture_uv(t, u_t, mode)
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), tex_oracle.sample_texture_uv(tex, uv, mode).view(np.uint32))
    out.backward(torch.from_numpy(g).to(gpu))
    want_t, want_uv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode)
    assert float(np.abs(t.grad.cpu().numpy() - want_t).max()) <= 2e-5 * max(1.0, float(np.abs(want_t).max()))
    assert float(np.abs(u_t.grad.cpu().numpy() - want_uv).max()) <= 1e-4 * max(1.0, float(np.abs(want_uv).max()))
    _, _, mass_t, mass_uv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, want_mass=True)
    _per_element(t.grad, want_t, mass_t, 'grad_texture')
    _per_element(u_t.grad, want_uv, mass_uv, 'grad_uvs')
    # nearest: the gradient of a gather
    t2 = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    texture.sample_texture_uv(t2, torch.from_numpy(uv).to(gpu), mode, 'nearest').backward(torch.from_numpy(g).to(gpu))
    t3 = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    texture.sample_texture(t3, texture.uvs_to_pixel_indices(torch.from_numpy(uv).to(gpu), t3.shape[:2], mode), 'nearest').backward(torch.from_numpy(g).to(gpu))
    assert torch.allclose(t2.grad, t3.grad, atol=2e-5 * max(1.0, float(t3.grad.abs().max())), rtol=1e-5)
    want_n, _, mass_n, _ = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, 'nearest', want_mass=True)   # ... and the oracle's
    _per_element(t2.grad, want_n, mass_n, 'nearest grad_texture')


# ---- per-element checks: the oracle's L1 mass of each element's terms (oracle/texture_oracle.py, want_mass=True) ----------

def test_oracle_mass_is_the_sum_of_the_terms_magnitudes():
    """want_mass=True: per texel and channel the sum of |g * w| over the look-ups touching it, per coordinate the terms of
    d_fc * dcol_du / d_fr * drow_dv with the texel differences over magnitudes -- recomputed here look-up by look-up from
    the plain gradient of each single look-up (the gradient is a sum over look-ups) and from the bilinear weights."""
    rng = np.random.default_rng(2)
    ht, wt, ct = 6, 5, 3
    tex = rng.uniform(-1, 1, (ht, wt, ct)).astype(np.float32)
    uv = rng.uniform(-0.3, 1.3, (17, 2)).astype(np.float32)
    uv[0] = [0.0, 0.0]; uv[1] = [1.0, 1.0]; uv[2] = [2.0 / wt, 3.0 / ht]
    g = rng.standard_normal((17, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        gt, guv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, want_mass=True)
        gt0, guv0 = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode)
        assert np.array_equal(gt, gt0) and np.array_equal(guv, guv0)
        assert mt.dtype == np.float64 and muv.dtype == np.float64 and mt.shape == tex.shape and muv.shape == uv.shape
        want_mt = np.zeros(tex.shape)
        want_muv = np.zeros(uv.shape)
        idx = tex_oracle._indices(uv, ht, wt, mode).astype(np.float64)
        for i in range(len(uv)):
            gi, _ = tex_oracle.sample_texture_uv_grad(tex, uv[i:i + 1], g[i:i + 1], mode)
            want_mt += np.abs(gi.astype(np.float64))           # one look-up: each texel's term is |g * w| (distinct taps)
            fr, fc = idx[i, 0] - np.floor(idx[i, 0]), idx[i, 1] - np.floor(idx[i, 1])
            r0, c0 = min(max(int(np.floor(idx[i, 0])), 0), ht - 1), min(max(int(np.floor(idx[i, 1])), 0), wt - 1)
            r1, c1 = min(r0 + 1, ht - 1), min(c0 + 1, wt - 1)
            t = np.abs(tex.astype(np.float64))
            ag = np.abs(g[i].astype(np.float64))
            du = wt if mode == 'repeat' or 0 <= uv[i, 0] <= 1 else 0
            dv = ht if mode == 'repeat' or 0 <= uv[i, 1] <= 1 else 0
            want_muv[i, 0] = (ag * ((t[r0, c1] + t[r0, c0]) * (1 - fr) + (t[r1, c1] + t[r1, c0]) * fr)).sum() * du
            want_muv[i, 1] = (ag * ((t[r1, c0] + t[r0, c0]) * (1 - fc) + (t[r1, c1] + t[r0, c1]) * fc)).sum() * dv
        # (where the taps of one look-up coincide -- the last row / column -- |sum| <= sum of ||: the mass may exceed;
        # `gi` is rounded to float32)
        inner = np.zeros(tex.shape, bool)
        inner[:-1, :-1] = True
        assert np.all(mt >= want_mt * (1 - 1e-6)) and np.allclose(mt[inner], want_mt[inner], rtol=1e-6, atol=1e-15)
        assert np.allclose(muv, want_muv, rtol=1e-12, atol=1e-15)
        assert np.all(np.abs(gt) <= mt * (1 + 1e-6) + 1e-12) and np.all(np.abs(guv) <= muv * (1 + 1e-6) + 1e-12)


def test_oracle_nearest_gradient_is_the_gather_scatter():
    """filter='nearest': dL/dtexture adds every look-up's grad_out into the texel it read (a finite difference over each texel is
    exact: the look-up is linear in the texture), dL/duv is zero; its mass is sum |g| per texel."""
    rng = np.random.default_rng(6)
    ht, wt, ct = 4, 7, 2
    tex = rng.uniform(0, 1, (ht, wt, ct)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (40, 2)).astype(np.float32)
    uv[0] = [1.0, 1.0]; uv[1] = [0.0, -0.0]; uv[2] = [3.0 / wt, 2.0 / ht]
    g = rng.standard_normal((40, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        gt, guv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, 'nearest', want_mass=True)
        assert not guv.any() and not muv.any()
        base = tex_oracle.sample_texture_uv(tex, uv, mode, 'nearest').astype(np.float64)
        for r in range(ht):
            for c in range(wt):
                t2 = tex.copy()
                t2[r, c] += 1.0
                hit = np.any(tex_oracle.sample_texture_uv(t2, uv, mode, 'nearest') != base, axis=-1)
                fd = ((tex_oracle.sample_texture_uv(t2, uv, mode, 'nearest') - base) * g).sum(0)
                assert np.allclose(gt[r, c], fd, rtol=1e-5, atol=1e-6), (mode, r, c)
                assert np.allclose(mt[r, c], np.abs(g[hit].astype(np.float64)).sum(0), rtol=1e-12), (mode, r, c)
        # the texel centres: nearest and bilinear read the same texel with weight 1
        rows, cols = np.meshgrid(np.arange(ht), np.arange(wt), indexing='ij')
        uvc = np.stack([cols / wt, rows / ht], -1).reshape(-1, 2).astype(np.float32)
        gc = rng.standard_normal((ht * wt, ct)).astype(np.float32)
        a = tex_oracle.sample_texture_uv_grad(tex, uvc, gc, mode, 'nearest')[0]
        b = tex_oracle.sample_texture_uv_grad(tex, uvc, gc, mode, 'bilinear')[0]
        assert np.allclose(a, gc.reshape(ht, wt, ct)) and np.allclose(a, b, atol=1e-6)


def test_oracle_non_finite_coordinates():
    """NaN / +-inf (u, v): `repeat` makes all three NaN indices (floor-mod), `clamp` saturates +-inf and keeps NaN
    (tf.clip_by_value); a NaN index blends NaN weights into texel (0, 0) and its neighbours."""
    tex = np.arange(12, dtype=np.float32).reshape(3, 4, 1) + 1
    uv = np.array([[np.nan, 0.5], [np.inf, 0.0], [-np.inf, 0.0], [0.5, np.nan]], np.float32)
    g = np.ones((4, 1), np.float32)
    rep = tex_oracle.sample_texture_uv(tex, uv, 'repeat')
    assert np.isnan(rep).all()
    cl = tex_oracle.sample_texture_uv(tex, uv, 'clamp')
    assert np.isnan(cl[0]).all() and np.isnan(cl[3]).all()
    assert cl[1, 0] == tex[0, 3, 0] and cl[2, 0] == tex[0, 0, 0]
    assert np.array_equal(tex_oracle.sample_texture_uv(tex, uv, 'clamp', 'nearest')[:, 0], [tex[1, 0, 0], tex[0, 3, 0], tex[0, 0, 0], tex[0, 2, 0]])
    gt, guv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv[:1], g[:1], 'clamp', want_mass=True)
    assert np.isnan(gt[1:3, 0:2]).all() and np.isfinite(np.delete(gt.reshape(-1), [4, 5, 8, 9])).all()
    assert guv[0, 0] == 0 and np.isnan(guv[0, 1])   # u: clip saturated (gradient 0 * finite); v: through u's NaN fraction


def _per_element(got, want, mass, what, tol=None):
    """|gpu - oracle| <= tol * mass per element (tests/parity.py's rule for the texture gradients; tol: parity.TIGHT_TOL), non-finite
    values in the same places; where the mass is 0 the GPU value must be exactly 0."""
    from tests import parity
    tol = parity.TIGHT_TOL if tol is None else tol
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want, mass = np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape == mass.shape, (what, got.shape, want.shape, mass.shape)
    bad_w = ~(np.isfinite(want) & np.isfinite(mass))
    bad_g = ~np.isfinite(got)
    assert np.array_equal(bad_w, bad_g), '%s: non-finite values in different places (%d oracle, %d gpu)' % (what, bad_w.sum(), bad_g.sum())
    ok = ~bad_w
    err, lim = np.abs(got - want)[ok], tol * mass[ok]
    if err.size and not np.all(err <= lim):
        worst = int(np.argmax(err - lim))
        raise AssertionError('%s: %d of %d elements outside %g * mass; worst err %g at mass %g (value %g)' % (
            what, int(np.sum(err > lim)), err.size, tol, err[worst], mass[ok][worst], want[ok][worst]))


def _forward_equal(got, want, what):
    """Bit for bit where the oracle is a number, NaN exactly where it is NaN (the payload of a NaN is not specified)."""
    got = got.detach().cpu().numpy()
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    assert np.array_equal(nan_w, nan_g), '%s: NaN in different places (%d oracle, %d gpu)' % (what, nan_w.sum(), nan_g.sum())
    assert np.array_equal(got[~nan_g].view(np.uint32), want[~nan_w].view(np.uint32)), '%s: differs from the oracle' % what


def _check_lookup(gpu, tex, uv, g, mode, filt, what, tex_t=None, uv_t=None, g_t=None, uv_grad_of=None):
    """Forward against the oracle, then both gradients per element against the oracle's, from tensors given or made here."""
    from dirt_amd import texture
    t = torch.from_numpy(tex).to(gpu) if tex_t is None else tex_t
    u = torch.from_numpy(uv).to(gpu) if uv_t is None else uv_t
    t.requires_grad_(True)
    leaf = u if uv_grad_of is None else uv_grad_of
    leaf.requires_grad_(True)
    if uv_grad_of is not None:
        u = uv_t()
    out = texture.sample_texture_uv(t, u, mode, filt)
    _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' forward')
    gt, guv = torch.autograd.grad(out, [t, leaf], torch.from_numpy(g).to(gpu) if g_t is None else g_t)
    want_t, want_uv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, filt, want_mass=True)
    _per_element(gt, want_t, mt, what + ' grad_texture')
    return guv, want_uv, muv


def _smooth_uv(B, H, W, scale, seed, seam=True):
    """A rotated, scaled (u, v) field per image (a rendered surface): `scale` texture widths across the frame; with `seam` it
    starts left of 0 so that `repeat` wraps inside the frame."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = []
    for _ in range(B):
        ang = rng.uniform(-0.4, 0.4)
        c, s = np.cos(ang), np.sin(ang)
        u = (c * xs / W + s * ys / H) * scale + (rng.uniform(-0.3, -0.1) if seam else 0.02)
        v = (-s * xs / W + c * ys / H) * scale + (rng.uniform(-0.2, 0.3) if seam else 0.03)
        out.append(np.stack([u, v], -1))
    return np.stack(out).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'nearest'])
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
@pytest.mark.parametrize('ct', [1, 2, 3, 4, 5, 8])
def test_gradients_per_element(gpu, ct, mode, filt):
    """Every channel-count specialisation (1, 3, 4) and the generic passes of four (2: one short pass; 5: a full and a short
    one; 8: two full ones), both wrap modes, both filters: a batch of a smooth field with a seam (patch and atomic tiles)
    and an image of random coordinates (atomic tiles); each gradient element within TIGHT_TOL of its own terms' mass."""
    rng = np.random.default_rng(100 + 10 * ct + (mode == 'clamp') * 2 + (filt == 'nearest'))
    Ht, Wt, H, W = 29, 43, 45, 70
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = np.concatenate([_smooth_uv(2, H, W, 1.3, ct), rng.uniform(-0.5, 1.5, (1, H, W, 2)).astype(np.float32)])
    g = rng.standard_normal((3, H, W, ct)).astype(np.float32)
    guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, filt, 'ct=%d %s %s' % (ct, mode, filt))
    _per_element(guv, want_uv, muv, 'grad_uvs')
    if filt == 'nearest':
        assert not guv.any()


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('smooth', [True, False])
def test_flat_list_backward(gpu, ct, smooth):
    """A flat [n, 2] list of look-ups: the backward kernel's 256 x 1 tiles (rows == 1), with a partial last tile; a smooth
    path through the texture (patch tiles) or random points (atomic tiles)."""
    rng = np.random.default_rng(7 + ct)
    n = 1000
    tex = rng.uniform(0, 1, (31, 22, ct)).astype(np.float32)
    if smooth:
        s = np.linspace(0, 1, n)
        uv = np.stack([0.1 + 0.05 * s + 0.01 * np.sin(40 * s), 0.9 - 0.06 * s], -1).astype(np.float32)
    else:
        uv = rng.uniform(-0.2, 1.2, (n, 2)).astype(np.float32)
    g = rng.standard_normal((n, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, 'bilinear', 'flat ct=%d %s' % (ct, mode))
        _per_element(guv, want_uv, muv, 'flat grad_uvs')


@pytest.mark.gpu
def test_four_channels_misaligned_take_the_generic_kernels(gpu):
    """Ct = 4 with `texture` and `grad_out` starting one float into their buffers (contiguous, 4 mod 16 bytes): the float4
    kernels do not apply, the generic ones run; values as the aligned case's."""
    rng = np.random.default_rng(9)
    Ht, Wt, H, W = 24, 40, 40, 48
    tex = rng.uniform(0, 1, (Ht, Wt, 4)).astype(np.float32)
    uv = _smooth_uv(1, H, W, 1.2, 9)[0]
    g = rng.standard_normal((H, W, 4)).astype(np.float32)
    tbuf = torch.zeros(Ht * Wt * 4 + 1, device=gpu)
    tbuf[1:] = torch.from_numpy(tex.reshape(-1)).to(gpu)
    t = tbuf[1:].view(Ht, Wt, 4).detach()
    gbuf = torch.zeros(H * W * 4 + 1, device=gpu)
    gbuf[1:] = torch.from_numpy(g.reshape(-1)).to(gpu)
    g_t = gbuf[1:].view(H, W, 4)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 and g_t.is_contiguous() and g_t.data_ptr() % 16 == 4
    for mode in ('repeat', 'clamp'):
        for filt in ('bilinear', 'nearest'):
            guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, filt, 'misaligned %s %s' % (mode, filt), tex_t=t, g_t=g_t)
            _per_element(guv, want_uv, muv, 'misaligned grad_uvs')


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4])
def test_uvs_in_place_from_an_odd_stride_gbuffer(gpu, ct):
    """(u, v) read in place from channels 2:4 of a 7-channel G-buffer: an odd element stride, so no 8-byte pair loads;
    the coordinates' gradient lands in those two channels only."""
    rng = np.random.default_rng(13 + ct)
    H, W = 37, 50
    tex = rng.uniform(0, 1, (26, 19, ct)).astype(np.float32)
    gbuf = rng.uniform(-0.3, 1.3, (2, H, W, 7)).astype(np.float32)
    gbuf[0, ..., 2:4] = _smooth_uv(1, H, W, 0.9, ct)[0]
    g = rng.standard_normal((2, H, W, ct)).astype(np.float32)
    gb = torch.from_numpy(gbuf).to(gpu)
    for mode in ('repeat', 'clamp'):
        guv, want_uv, muv = _check_lookup(gpu, tex, gbuf[..., 2:4], g, mode, 'bilinear', 'gbuffer ct=%d %s' % (ct, mode),
                                          uv_t=lambda: gb[..., 2:4], uv_grad_of=gb)
        guv = guv.cpu().numpy()
        assert not guv[..., :2].any() and not guv[..., 4:].any()
        _per_element(guv[..., 2:4], want_uv, muv, 'gbuffer grad_uvs')


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('texels_per_pixel', [1.5, 8.0])
def test_minified_smooth_fields(gpu, ct, texels_per_pixel):
    """A smooth field without seams at 1.5 texels per pixel (a 16 x 16 tile's patch ~26 x 26 texels: well inside TEX_PATCH =
    1600) and at 8 (~130 x 130 texels: smooth, but too large for the LDS patch: the atomic path)."""
    rng = np.random.default_rng(17 + ct)
    H, W = 48, 64
    Wt = Ht = int(np.ceil(texels_per_pixel * W * 1.1))
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = _smooth_uv(1, H, W, texels_per_pixel * W / Wt, 20 + ct, seam=False)
    g = rng.standard_normal((1, H, W, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, 'bilinear', 'minified ct=%d x%g %s' % (ct, texels_per_pixel, mode))
        _per_element(guv, want_uv, muv, 'minified grad_uvs')


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 17), (13, 1), (1, 1)])
@pytest.mark.parametrize('ct', [1, 4])
def test_one_texel_wide_textures(gpu, shape, ct):
    """1 x Wt, Ht x 1 and 1 x 1 textures: the second tap of the short axis is the first (clamped); its texel difference is 0."""
    rng = np.random.default_rng(23)
    tex = rng.uniform(0, 1, shape + (ct,)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (2, 33, 40, 2)).astype(np.float32)
    g = rng.standard_normal((2, 33, 40, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        for filt in ('bilinear', 'nearest'):
            guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, filt, 'texture %s ct=%d %s %s' % (shape, ct, mode, filt))
            _per_element(guv, want_uv, muv, 'grad_uvs')


def _edge_and_special_uvs(Ht, Wt, rng):
    vals = [0.0, -0.0, 1.0, 0.5, 1.0 - 2 ** -24, -2 ** -24, 2.0, -1.0] + [k / Wt for k in range(0, Wt + 1, 3)] + [k / Ht for k in range(0, Ht + 1, 2)]
    vals = np.asarray(vals, np.float32)
    u, v = np.meshgrid(vals, vals[::-1])
    return np.stack([u, v], -1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_coordinates_on_texel_edges(gpu, ct):
    """(u, v) exactly at 0, -0.0, 1, just below 1 / above -0, whole multiples of 1 (repeat) and on every texel edge k / Wt:
    where the floor, the fraction, the last-texel rule and clip_by_value's gradient switch."""
    rng = np.random.default_rng(31)
    Ht, Wt = 10, 14
    tex = rng.uniform(0, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = _edge_and_special_uvs(Ht, Wt, rng)
    g = rng.standard_normal(uv.shape[:-1] + (ct,)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        for filt in ('bilinear', 'nearest'):
            guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, filt, 'edges ct=%d %s %s' % (ct, mode, filt))
            _per_element(guv, want_uv, muv, 'edge grad_uvs')


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_non_finite_coordinates(gpu, ct):
    """NaN and +-inf in u and / or v, in both modes and filters (the rule: oracle/texture_oracle.py::sample_texture_uv_grad):
    the look-up equals the oracle bit for bit with NaN in the same places, and the gradients are non-finite in the same
    places and within tolerance elsewhere -- in a smooth field (patch tiles) and in a random one."""
    rng = np.random.default_rng(41 + ct)
    Ht, Wt, H, W = 21, 30, 34, 48
    tex = rng.uniform(0, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = np.concatenate([_smooth_uv(1, H, W, 0.5, 3, seam=False), rng.uniform(-0.5, 1.5, (1, H, W, 2)).astype(np.float32)])
    specials = [(np.nan, 0.3), (0.3, np.nan), (np.nan, np.nan), (np.inf, 0.4), (-np.inf, 0.4), (0.4, np.inf), (0.4, -np.inf),
                (np.inf, -np.inf), (np.nan, np.inf)]
    for b in range(2):
        for k, (a, c) in enumerate(specials):
            uv[b, 5 + 3 * k, 7 + 4 * k] = (a, c)
    g = rng.standard_normal((2, H, W, ct)).astype(np.float32)
    for mode in ('repeat', 'clamp'):
        for filt in ('bilinear', 'nearest'):
            guv, want_uv, muv = _check_lookup(gpu, tex, uv, g, mode, filt, 'non-finite ct=%d %s %s' % (ct, mode, filt))
            _per_element(guv, want_uv, muv, 'non-finite grad_uvs')
