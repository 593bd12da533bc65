"""The trilinear (mipmapped) texture look-up (dirt_amd.texture.sample_texture_uv(filter='trilinear'), mip_pyramid;
include/dirt_hip.h dirt_texture_mip_* / dirt_texture_sample_mip_*) against the numpy restatement of DESIGN.md §7
(tests/mip_reference.py), and the restatement itself against hand-computed values and finite differences on the CPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mip_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # per element, relative to the L1 mass of the element's terms (forward: to the value's magnitude)


# ---- the restatement, on the CPU ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,levels', [((512, 512), 10), ((480, 640), 6), ((8, 2), 4), ((6, 9), 1), ((1, 1), 1)])
def test_reference_level_counts(shape, levels):
    assert mr.level_count(*shape) == levels
    pyr = mr.pyramid(np.zeros(shape + (2,), np.float32))
    assert len(pyr) == levels
    if shape == (480, 640):
        assert pyr[-1].shape[:2] == (15, 20)
    assert mr.level_count(512, 512, max_level=3) == 4 and mr.level_count(512, 512, max_level=0) == 1


def test_reference_pyramid_means():
    assert all(np.all(p == np.float32(0.37)) for p in mr.pyramid(np.full((16, 4, 3), 0.37, np.float32)))
    t = np.array([[1., 2.], [3., 5.]], np.float32)[..., None]
    assert mr.pyramid(t)[1][0, 0, 0] == np.float32(((1 + 2) + (3 + 5)) * 0.25)
    col = np.array([[1.], [4.], [2.], [8.]], np.float32)[..., None]     # 4 x 1: 2 x 1 means down the rows
    p = mr.pyramid(col)
    assert [q.shape[:2] for q in p] == [(4, 1), (2, 1), (1, 1)]
    assert p[1][:, 0, 0].tolist() == [2.5, 5.0] and p[2][0, 0, 0] == 3.75
    p = mr.pyramid(np.array([[1., 3., 6., 10.]], np.float32)[..., None])  # 1 x 4: along the row
    assert p[1][0, :, 0].tolist() == [2.0, 8.0] and p[2][0, 0, 0] == 5.0


@pytest.mark.parametrize('s', [1, 2, 4, 8])
def test_reference_lod_of_an_affine_image(s):
    ht, wt, H, W = 256, 512, 24, 40
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    uv = np.stack([0.1 + xs * s / wt, 0.2 + ys * 0.5 / ht], -1).astype(np.float32)
    lam = mr.footprint_lod(uv, ht, wt, 'clamp')
    assert np.allclose(lam, np.log2(s), atol=1e-4), (lam.min(), lam.max())
    assert np.allclose(mr.footprint_lod(uv, ht, wt, 'clamp', lod_bias=-0.5), np.log2(s) - 0.5, atol=1e-4)


def test_reference_gradients_are_finite_differences():
    rng = np.random.default_rng(5)
    tex = rng.uniform(-1, 1, (16, 8, 3)).astype(np.float32)
    uv = rng.uniform(-0.2, 1.2, (2, 5, 7, 2)).astype(np.float32)
    lod = rng.uniform(-0.5, 4.5, (2, 5, 7)).astype(np.float32)
    g = rng.standard_normal((2, 5, 7, 3))
    for mode in ('repeat', 'clamp'):
        r = mr.grad(tex, uv, g, mode, lod=lod, lod_bias=0.25)

        def loss(t=tex, u=uv, l=lod):
            return float((mr.sample(t, u, mode, lod=l, lod_bias=0.25, dtype=np.float64) * g).sum())
        t64, u64, l64 = tex.astype(np.float64), uv.astype(np.float64), lod.astype(np.float64)
        for idx in [(0, 0, 0), (3, 2, 1), (15, 7, 2), (8, 4, 0)]:
            tp, tm = t64.copy(), t64.copy()
            tp[idx] += 1e-4; tm[idx] -= 1e-4
            fd = (loss(t=tp) - loss(t=tm)) / 2e-4
            assert abs(fd - r['grad_texture'][idx]) <= 1e-6 * max(1.0, r['mass_texture'][idx]), (mode, idx, fd, r['grad_texture'][idx])
        for idx in [(0, 1, 2, 0), (1, 3, 4, 1), (0, 4, 6, 0), (1, 0, 0, 1)]:
            up, um = u64.copy(), u64.copy()
            up[idx] += 1e-7; um[idx] -= 1e-7
            fd = (loss(u=up) - loss(u=um)) / 2e-7
            assert abs(fd - r['grad_uvs'][idx]) <= 1e-4 * max(1.0, r['mass_uvs'][idx]), (mode, idx, fd, r['grad_uvs'][idx])
        for idx in [(0, 1, 2), (1, 3, 4), (0, 4, 6), (1, 2, 5)]:
            lp, lm = l64.copy(), l64.copy()
            lp[idx] += 1e-6; lm[idx] -= 1e-6
            fd = (loss(l=lp) - loss(l=lm)) / 2e-6
            assert abs(fd - r['grad_lod'][idx]) <= 1e-5 * max(1.0, r['mass_lod'][idx]), (mode, idx, fd, r['grad_lod'][idx])


def test_argument_checks_without_a_gpu():
    from dirt_amd import texture as tx
    t, uv = torch.zeros(8, 8, 3), torch.zeros(5, 2)
    with pytest.raises(ValueError):
        tx.sample_texture_uv(t, uv, filter='trilinear')                       # a flat list has no neighbours: lod needed
    for kw in ({'lod': torch.zeros(5)}, {'lod_bias': 1.0}, {'mask': torch.ones(5)}, {'max_level': 2}):
        for filt in ('bilinear', 'nearest'):
            with pytest.raises(ValueError):
                tx.sample_texture_uv(t, uv, filter=filt, **kw)
    for filt in ('bilinear', 'trilinear'):
        with pytest.raises(ValueError):
            tx.sample_texture_uv(t, torch.zeros(4, 5, 3), filter=filt)         # [..., 3] coordinates
        with pytest.raises(ValueError):
            tx.sample_texture_uv(torch.zeros(8, 8), torch.zeros(4, 5, 2), filter=filt)
    img = torch.zeros(4, 5, 2)
    with pytest.raises(ValueError):
        tx.sample_texture_uv(t, img, filter='trilinear', lod=torch.zeros(4, 4))  # lod not shaped like uvs[..., 0]
    with pytest.raises(ValueError):
        tx.sample_texture_uv(t, img, filter='trilinear', mask=torch.ones(5, 4))
    with pytest.raises(ValueError):
        tx.sample_texture_uv(t, img, filter='trilinear', max_level=-1)
    with pytest.raises(ValueError):
        tx.mip_pyramid(torch.zeros(8, 8))


# ---- the kernels against the restatement, on the GPU ------------------------------------------------------------------

def _bits_equal(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), '%s: %d elements differ' % (what, int(np.sum(got != want)))


def _per_element(got, want, mass, what, tol=TOL):
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want, mass = np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape == mass.shape, (what, got.shape, want.shape, mass.shape)
    assert np.isfinite(got).all(), what
    err, lim = np.abs(got - want), tol * mass + 1e-30
    if not np.all(err <= lim):
        worst = int(np.argmax(err - lim))
        raise AssertionError('%s: %d of %d elements outside %g * mass; worst err %g at mass %g (value %g)' % (
            what, int(np.sum(err > lim)), err.size, tol, err.flat[worst], mass.flat[worst], want.flat[worst]))


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


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(512, 512, 1), (512, 512, 3), (512, 512, 4), (480, 640, 3), (8, 2, 5), (1, 1, 2)])
def test_pyramid_is_bit_exact(gpu, shape):
    from dirt_amd import texture
    tex = np.random.default_rng(sum(shape)).uniform(-1, 1, shape).astype(np.float32)
    got = texture.mip_pyramid(torch.from_numpy(tex).to(gpu))
    want = mr.pyramid(tex)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        _bits_equal(a, b, 'level %d of %s' % (k, shape))
    assert len(texture.mip_pyramid(torch.from_numpy(tex).to(gpu), max_level=2)) == min(3, len(want))


@pytest.mark.gpu
def test_pyramid_backward_is_the_gradient_of_a_2x2_average(gpu):
    from dirt_amd import texture
    rng = np.random.default_rng(8)
    for shape in ((64, 32, 3), (16, 2, 1), (8, 8, 4)):
        t = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(gpu).requires_grad_(True)
        levels = texture.mip_pyramid(t)
        gs = [torch.from_numpy(rng.standard_normal(tuple(lv.shape)).astype(np.float32)).to(gpu) for lv in levels]
        sum(float(1) * (lv * g).sum() for lv, g in zip(levels, gs)).backward()
        t2 = t.detach().clone().requires_grad_(True)
        lv, loss = t2, (t2 * gs[0]).sum()
        for g in gs[1:]:
            x = lv.permute(2, 0, 1)[None]
            kh, kw = (2 if lv.shape[0] > 1 else 1), (2 if lv.shape[1] > 1 else 1)
            lv = torch.nn.functional.avg_pool2d(x, (kh, kw))[0].permute(1, 2, 0)
            loss = loss + (lv * g).sum()
        loss.backward()
        assert torch.allclose(t.grad, t2.grad, rtol=1e-5, atol=1e-5), float((t.grad - t2.grad).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_trilinear_at_lod_zero_or_magnified_is_bilinear_bit_for_bit(gpu, ct):
    from dirt_amd import texture
    rng = np.random.default_rng(30 + ct)
    tex = torch.from_numpy(rng.uniform(0, 1, (64, 128, ct)).astype(np.float32)).to(gpu)
    uv = torch.from_numpy(rng.uniform(-0.5, 1.5, (40, 56, 2)).astype(np.float32)).to(gpu)
    mag = torch.from_numpy(_smooth_uv(2, 48, 64, 0.3, ct)).to(gpu)     # ~0.2-0.6 texels per pixel: lambda < 0
    for mode in ('repeat', 'clamp'):
        bil = texture.sample_texture_uv(tex, uv, mode)
        tri = texture.sample_texture_uv(tex, uv, mode, 'trilinear', lod=torch.zeros(40, 56, device=gpu))
        assert torch.equal(bil.view(torch.int32), tri.view(torch.int32))
        bil = texture.sample_texture_uv(tex, mag, mode)
        tri = texture.sample_texture_uv(tex, mag, mode, 'trilinear')
        assert torch.equal(bil.view(torch.int32), tri.view(torch.int32))


def _forward_close(got, tex, uv, what, **kw):
    want, mag = mr.sample(tex, uv, magnitude=True, **kw)
    got = got.detach().cpu().numpy()
    _per_element(got, want, mag, what + ' forward')


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
def test_forward_matches_the_restatement(gpu, ct, mode):
    from dirt_amd import texture
    rng = np.random.default_rng(40 + ct + 7 * (mode == 'clamp'))
    Ht, Wt, H, W = 128, 64, 37, 50
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    t = torch.from_numpy(tex).to(gpu)
    # three images whose fields jump from one to the next (minified 0.5x to 6x): neighbours must not cross images
    uv = np.concatenate([_smooth_uv(1, H, W, s, ct + i, (0.1 * i, -0.2)) for i, s in enumerate((0.4, 3.0, 9.0))])
    u = torch.from_numpy(uv).to(gpu)
    _forward_close(texture.sample_texture_uv(t, u, mode, 'trilinear'), tex, uv, 'plain', mode=mode)
    _forward_close(texture.sample_texture_uv(t, u, mode, 'trilinear', lod_bias=0.7, max_level=3), tex, uv, 'bias+max_level',
                   mode=mode, lod_bias=0.7, max_level=3)
    # (u, v) and mask read in place from a G-buffer [B, H, W, 6]: mask channel 0, (u, v) channels 1:3
    gbuf = np.zeros((3, H, W, 6), np.float32)
    gbuf[..., 1:3] = uv
    gbuf[..., 0] = (rng.uniform(0, 1, (3, H, W)) > 0.3).astype(np.float32)
    gb = torch.from_numpy(gbuf).to(gpu)
    got = texture.sample_texture_uv(t, gb[..., 1:3], mode, 'trilinear', mask=gb[..., 0], lod_bias=-0.3)
    _forward_close(got, tex, uv, 'mask', mode=mode, mask=gbuf[..., 0], lod_bias=-0.3)
    # explicit lod on a flat list (beyond both ends of the pyramid too)
    flat = rng.uniform(-0.3, 1.3, (777, 2)).astype(np.float32)
    lod = rng.uniform(-1, 9, 777).astype(np.float32)
    got = texture.sample_texture_uv(t, torch.from_numpy(flat).to(gpu), mode, 'trilinear', lod=torch.from_numpy(lod).to(gpu))
    _forward_close(got, tex, flat, 'explicit lod', mode=mode, lod=lod)


def _check_grads(gpu, tex, uv, g, what, mode='repeat', lod=None, **kw):
    from dirt_amd import texture
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    u = torch.from_numpy(uv).to(gpu).requires_grad_(True)
    leaves = [t, u]
    lt = None
    if lod is not None:
        lt = torch.from_numpy(lod).to(gpu).requires_grad_(True)
        leaves.append(lt)
    out = texture.sample_texture_uv(t, u, mode, 'trilinear', lod=lt, **kw)
    _forward_close(out, tex, uv, what, mode=mode, lod=lod, **kw)
    grads = torch.autograd.grad(out, leaves, torch.from_numpy(g).to(gpu))
    r = mr.grad(tex, uv, g, mode, lod=lod, **kw)
    _per_element(grads[0], r['grad_texture'], r['mass_texture'], what + ' grad_texture')
    _per_element(grads[1], r['grad_uvs'], r['mass_uvs'], what + ' grad_uvs')
    if lod is not None:
        _per_element(grads[2], r['grad_lod'], r['mass_lod'], what + ' grad_lod')
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
def test_gradients_of_a_smooth_gbuffer_patch_path(gpu, ct, mode):
    """Smooth fields at 0.5x to 5x minification: 16 x 16 tiles touch one or two adjacent levels (the LDS patches)."""
    rng = np.random.default_rng(60 + ct)
    Ht, Wt, H, W = 256, 128, 45, 70
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = np.concatenate([_smooth_uv(1, H, W, s, 3 * ct + i) for i, s in enumerate((0.4, 2.5, 5.0))])
    g = rng.standard_normal((3, H, W, ct)).astype(np.float32)
    _check_grads(gpu, tex, uv, g, 'smooth ct=%d %s' % (ct, mode), mode)
    _check_grads(gpu, tex, uv, g, 'smooth+bias ct=%d %s' % (ct, mode), mode, lod_bias=0.6, max_level=4)


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
@pytest.mark.parametrize('mode', ['repeat', 'clamp'])
def test_gradients_of_scattered_lookups_fallback_path(gpu, ct, mode):
    """Random coordinates with an explicit, random lod: every tile spans many levels and texels (float atomics into the
    scratch pyramid); lod gradients included, and lods outside [0, L - 1] (zero lod gradient)."""
    rng = np.random.default_rng(80 + ct)
    tex = rng.uniform(-1, 1, (64, 32, ct)).astype(np.float32)
    uv = rng.uniform(-0.3, 1.3, (2, 20, 33, 2)).astype(np.float32)
    lod = rng.uniform(-1, 7.5, (2, 20, 33)).astype(np.float32)
    lod[0, 0, :4] = [0.0, 2.0, 6.0, 3.0]
    g = rng.standard_normal((2, 20, 33, ct)).astype(np.float32)
    _check_grads(gpu, tex, uv, g, 'scattered ct=%d %s' % (ct, mode), mode, lod=lod)
    flat = uv.reshape(-1, 2)[:500]
    _check_grads(gpu, tex, flat, g.reshape(-1, ct)[:500], 'flat ct=%d %s' % (ct, mode), mode, lod=lod.reshape(-1)[:500], lod_bias=-0.4)


@pytest.mark.gpu
def test_gradients_with_a_mask_read_in_place(gpu):
    from dirt_amd import texture
    rng = np.random.default_rng(99)
    tex = rng.uniform(-1, 1, (128, 128, 3)).astype(np.float32)
    H, W = 40, 52
    gbuf = np.zeros((2, H, W, 6), np.float32)
    gbuf[..., 1:3] = _smooth_uv(2, H, W, 3.0, 5)
    gbuf[..., 0] = (rng.uniform(0, 1, (2, H, W)) > 0.25).astype(np.float32)
    g = rng.standard_normal((2, H, W, 3)).astype(np.float32)
    t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
    gb = torch.from_numpy(gbuf).to(gpu).requires_grad_(True)
    out = texture.sample_texture_uv(t, gb[..., 1:3], 'repeat', 'trilinear', mask=gb[..., 0])
    gt, ggb = torch.autograd.grad(out, [t, gb], torch.from_numpy(g).to(gpu))
    r = mr.grad(tex, gbuf[..., 1:3], g, 'repeat', mask=gbuf[..., 0])
    _per_element(gt, r['grad_texture'], r['mass_texture'], 'mask grad_texture')
    ggb = ggb.cpu().numpy()
    _per_element(ggb[..., 1:3], r['grad_uvs'], r['mass_uvs'], 'mask grad_uvs')
    assert not ggb[..., 0].any() and not ggb[..., 3:].any()


@pytest.mark.gpu
def test_minified_texture_every_texel_gets_gradient_and_aliasing_drops(gpu):
    """640 x 480 pixels over a 2048 x 2048 noise texture at 4x minification (the left 508 columns are surface, the rest
    background with no gradient): bilinear reads 4 of every 16 texels -- ~75 % of the texels under the surface get no
    gradient and the image aliases; trilinear reaches all of them and stays close to the box-filtered texture."""
    from dirt_amd import texture
    rng = np.random.default_rng(123)
    Ht = Wt = 2048
    H, W, S = 480, 640, 508
    tex = rng.uniform(0, 1, (Ht, Wt, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    gbuf = np.zeros((H, W, 6), np.float32)
    gbuf[..., 1] = (4 * xs + 0.5 + 8) / Wt
    gbuf[..., 2] = (4 * ys + 0.5 + 8) / Ht
    gbuf[..., 0] = xs < S
    gb = torch.from_numpy(gbuf).to(gpu)
    mask = gb[..., :1]
    g = torch.from_numpy(rng.standard_normal((H, W, 3)).astype(np.float32)).to(gpu) * mask
    region = (slice(8 + 8, 8 + 4 * H - 8), slice(8 + 8, 8 + 4 * S - 8))     # texels under the surface, borders excluded
    box = tex[8:8 + 4 * H, 8:8 + 4 * S].reshape(H, 4, S, 4, 3).mean((1, 3))  # ground truth: each pixel's 4 x 4 texels
    errs = {}
    for filt in ('bilinear', 'trilinear'):
        t = torch.from_numpy(tex).to(gpu).requires_grad_(True)
        kw = {'mask': gb[..., 0]} if filt == 'trilinear' else {}
        out = texture.sample_texture_uv(t, gb[..., 1:3], 'repeat', filt, **kw)
        out.backward(g)
        zero = (t.grad[region].abs().sum(-1) == 0).float().mean().item()
        if filt == 'bilinear':
            assert zero >= 0.6, zero
        else:
            assert zero == 0.0, zero
        errs[filt] = float(((out.detach()[:, :S].cpu().numpy() - box) ** 2).mean())
    assert errs['trilinear'] < 0.5 * errs['bilinear'], errs


@pytest.mark.gpu
def test_end_to_end_rasterise_deferred_with_a_trilinear_shader(gpu):
    spec = importlib.util.spec_from_file_location('textured_mip_example', os.path.join(ROOT, 'examples', 'textured_mip.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    pixels, texture, light, vertices = ex.run(gpu, 'trilinear')
    assert torch.isfinite(pixels).all()
    for name, x in (('texture', texture), ('light', light), ('vertices', vertices)):
        assert x.grad is not None and torch.isfinite(x.grad).all(), name
        assert x.grad.abs().sum().item() > 0, name
