"""The restatement `dirt_amd.shading.shade_gbuffer_sh` is checked against: `dirt_amd.lighting.spherical_harmonics` on CPU
tensors, the mask composite and the clamp of DESIGN.md §7b, gradients by torch's autograd.  Coefficients and background are
expanded to one row per pixel and made leaves: a parameter's gradient is the sum of its leaf's rows, its L1 mass the sum of
their absolute values.  Run in float64 it is the reference; run in float32 it is the composition users had before the
kernel, whose error sets the tolerance (`measure_f32`).

The L1 mass of an element is taken per basis term and output channel (27 terms and the background's three), and inside the
normalisation per autograd path: |n| is taken of a detached leaf copy of the normals, so the half of d (n / |n|) / d n that
flows through the norm arrives there and the direct half at the normals -- the two cancel along n.

    python -m tests.shade_sh_reference      # prints the float32 figures the constants of tests/test_shade_sh.py restate
"""
import numpy as np
import torch

from dirt_amd import lighting
from tests.shade_reference import worst_ratio

C0 = lighting.SH_C0
LAMBERT = lighting.SH_LAMBERT


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)).to(dtype)


def compose(gbuffer, coefficients, layout, colors=None, background=(0., 0., 0.), clamp=(0., 1.), normalize=False, band_scale=(1., 1., 1.),
            grad_out=None, scene_index=None, dtype=torch.float64, masses=True):
    """gbuffer [N, Cg] (float32 values); coefficients [K, 3] or [R, K, 3] and background [3] or [R, 3] with scene_index [N]
    (pixel -> row); layout: dict(colors=, normals=, mask=) of first channels (colors absent with `colors` [N, 3] given).
    -> dict: out, pre; with grad_out [N, 3] also d_gbuffer, d_colors, d_normals, d_mask ([N, 0] without a mask), d_coefficients
    [R, K, 3], d_background [R, 3]; with masses also mass_out and mass_<each of those>."""
    g = _t(gbuffer, dtype).requires_grad_(True)
    n_px = g.shape[0]
    idx = torch.zeros(n_px, dtype=torch.long) if scene_index is None else torch.as_tensor(np.asarray(scene_index)).long()
    col = _t(colors, dtype).requires_grad_(True) if colors is not None else None
    table = _t(coefficients, dtype)
    table = table.reshape((-1,) + tuple(table.shape[-2:]))
    ground = _t(background, dtype).reshape(-1, 3)
    at = lambda shared: idx if shared.shape[0] > 1 else torch.zeros_like(idx)   # noqa: E731
    L = table[at(table)].clone().requires_grad_(True)       # [N, K, 3]
    bg = ground[at(ground)].clone().requires_grad_(True)    # [N, 3]

    def parts(gb, cl):
        c = cl if cl is not None else gb[:, layout['colors']:layout['colors'] + 3]
        n = gb[:, layout['normals']:layout['normals'] + 3]
        m = gb[:, layout['mask']:layout['mask'] + 1] if layout.get('mask') is not None else torch.ones(n_px, 1, dtype=dtype)
        return c, n, m

    c, n, m = parts(g, col)
    lit = lighting.spherical_harmonics(n[:, None], c[:, None], L, band_scale=band_scale, normalize=normalize)[:, 0]
    pre = lit * m + bg * (1. - m)
    out = torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre
    res = {'out': out.detach(), 'pre': pre.detach()}
    sl_n = slice(layout['normals'], layout['normals'] + 3)
    sl_m = slice(layout['mask'], layout['mask'] + 1) if layout.get('mask') is not None else slice(0, 0)

    def split(d_g, d_col):
        d_c = d_col if col is not None else d_g[:, layout['colors']:layout['colors'] + 3]
        return d_c, d_g[:, sl_n], d_g[:, sl_m]

    if grad_out is not None:
        go = _t(grad_out, dtype)
        leaves = [g, L, bg] + ([col] if col is not None else [])
        grads = torch.autograd.grad((out * go).sum(), leaves, allow_unused=True)
        grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
        res['d_gbuffer'] = grads[0]
        res['d_colors'], res['d_normals'], res['d_mask'] = split(grads[0], grads[3] if col is not None else None)
        for name, shared, gr in (('coefficients', table, grads[1]), ('background', ground, grads[2])):
            res['d_' + name] = torch.zeros_like(shared).index_add_(0, at(shared), gr)
            res['mass_' + name] = torch.zeros_like(shared).index_add_(0, at(shared), gr.abs())
    if not masses:
        return res

    # ---- L1 masses: every term apart, the normalisation's two halves apart
    gm = g.detach().clone().requires_grad_(True)
    cm = col.detach().clone().requires_grad_(True) if col is not None else None
    c, n, m = parts(gm, cm)
    n_leaf = n.detach().clone().requires_grad_(True)
    nh = n / torch.linalg.vector_norm(n_leaf, dim=-1, keepdim=True).clamp_min(1.e-12) if normalize else n
    K = L.shape[1]
    Y = lighting.sh_basis(nh)[:, :K] * torch.tensor([float(band_scale[b]) for b in lighting.SH_BAND[:K]], dtype=dtype)
    Ld, bgd = L.detach(), bg.detach()
    terms = [(j, c[:, j] * Y[:, k] * Ld[:, k, j] * m[:, 0]) for k in range(K) for j in range(3)]
    terms += [(j, bgd[:, j] * (1. - m[:, 0])) for j in range(3)]
    res['mass_out'] = torch.zeros(n_px, 3, dtype=dtype)
    for j, q in terms:
        res['mass_out'][:, j] += q.detach().abs()
    if grad_out is None:
        return res
    gate = ((pre >= clamp[0]) & (pre <= clamp[1])).to(dtype).detach() if clamp is not None else torch.ones_like(pre).detach()
    mass_g = torch.zeros_like(gm)
    mass_c = torch.zeros(n_px, 3, dtype=dtype)
    leaves = [gm] + ([cm] if cm is not None else []) + ([n_leaf] if normalize else [])
    for j, q in terms:
        if not q.requires_grad:   # the background's term without a mask channel
            continue
        grads = list(torch.autograd.grad((gate[:, j] * go[:, j] * q).sum(), leaves, retain_graph=True, allow_unused=True))
        d_g = grads.pop(0)
        if d_g is not None:
            mass_g += d_g.abs()
        if cm is not None:
            d_c = grads.pop(0)
            if d_c is not None:
                mass_c += d_c.abs()
        if normalize and grads[0] is not None:
            mass_g[:, sl_n] += grads[0].abs()
    res['mass_gbuffer'] = mass_g
    res['mass_colors'], res['mass_normals'], res['mass_mask'] = split(mass_g, mass_c if cm is not None else None)
    return res


def off_kinks(res, clamp, margin=1.e-3):
    """[N] bool: the pixel's pre-clamp values are at least `margin` from lo and hi."""
    if clamp is None:
        return torch.ones(res['pre'].shape[0], dtype=torch.bool)
    return ((res['pre'] - clamp[0]).abs() >= margin).all(1) & ((res['pre'] - clamp[1]).abs() >= margin).all(1)


def random_coefficients(rng, K=9, batch=None, factor=1.):
    """N(0, 0.3), band 0 set to U(0.8, 1.6) * 0.5 / C0 (a pixel's irradiance sits around 0.4-0.8); `factor` multiplies the table."""
    shape = (K, 3) if batch is None else (batch, K, 3)
    L = rng.normal(0., 0.3, shape)
    L[..., 0, :] = rng.uniform(0.8, 1.6, shape[:-2] + (3,)) * 0.5 / C0
    return (L * factor).astype(np.float32)


def random_pixels(rng, n, cg, layout, unit_normals=True, tensor_colors=False, covered=0.7):
    """(gbuffer [n, cg], colors [n, 3] or None): colours U(0.05, 1), normals unit vectors or (for normalize=True) standard-normal
    vectors, a mask of 0 / 1 / fractional coverage (70 % / 10 % fractional); the channels no attribute uses hold noise."""
    g = rng.standard_normal((n, cg)).astype(np.float32)
    col = rng.uniform(0.05, 1., (n, 3)).astype(np.float32)
    if not tensor_colors:
        g[:, layout['colors']:layout['colors'] + 3] = col
    nn = rng.standard_normal((n, 3))
    g[:, layout['normals']:layout['normals'] + 3] = nn / np.linalg.norm(nn, axis=1, keepdims=True) if unit_normals else nn
    if layout.get('mask') is not None:
        u = rng.uniform(0., 1., n)
        g[:, layout['mask']] = np.where(u < covered, 1., np.where(u < covered + 0.1, rng.uniform(0.1, 0.9, n), 0.))
    return g, (col if tensor_colors else None)


def draw_off_kinks(rng, n, cg, layout, coefficients, kw, tensor_colors=False, scene_index=None, max_rejected=0.05):
    """Random pixels that all stay off the clamp's edges: draw, reject against the float64 restatement, redraw the rejected
    pixels.  The share rejected from the first draw must stay under `max_rejected`.  -> (gbuffer, colors or None, share)"""
    unit = not kw.get('normalize', False)
    g, col = random_pixels(rng, n, cg, layout, unit, tensor_colors)
    share = None
    for _ in range(20):
        ref = compose(g, coefficients, layout, colors=col, scene_index=scene_index, masses=False, **kw)
        bad = ~off_kinks(ref, kw.get('clamp', (0., 1.))).numpy()
        if share is None:
            share = float(bad.mean())
            assert share < max_rejected, 'share of rejected pixels %.3f' % share
        if not bad.any():
            return g, col, share
        g[bad], c2 = random_pixels(rng, int(bad.sum()), cg, layout, unit, tensor_colors)
        if tensor_colors:
            col[bad] = c2
    raise AssertionError('could not draw pixels off the kinks')


KINDS = ('pixels', 'd_colors', 'd_normals', 'd_mask', 'd_params')


def ratios(got, ref):
    """The worst |got - ref| / mass per kind of result; got: dict with out, d_colors, d_normals, d_mask, d_coefficients,
    d_background (entries that are missing or None are skipped), ref: `compose(..., masses=True)`."""
    worst = {}
    pairs = (('pixels', 'out', 'mass_out'), ('d_colors', 'd_colors', 'mass_colors'), ('d_normals', 'd_normals', 'mass_normals'),
             ('d_mask', 'd_mask', 'mass_mask'), ('d_params', 'd_coefficients', 'mass_coefficients'),
             ('d_params', 'd_background', 'mass_background'))
    for kind, key, mass in pairs:
        if got.get(key) is None or key not in ref:
            continue
        a = np.asarray(got[key].detach().cpu() if isinstance(got[key], torch.Tensor) else got[key], dtype=np.float64).reshape(ref[key].shape)
        worst[kind] = max(worst.get(kind, 0.), worst_ratio(a, ref[key].numpy(), ref[mass].numpy()))
    return worst


def measure_f32(cases):
    """cases: iterable of (positional arguments, keyword arguments) of `compose` -> the worst |f32 - f64| / mass of the float32
    composition per kind of result (KINDS)."""
    worst = dict.fromkeys(KINDS, 0.)
    for args, kw in cases:
        r64 = compose(*args, dtype=torch.float64, **kw)
        r32 = compose(*args, dtype=torch.float32, masses=False, **kw)
        for k, v in ratios(r32, r64).items():
            worst[k] = max(worst[k], v)
    return worst


if __name__ == '__main__':
    from tests import test_shade_sh
    print({k: '%.3e' % v for k, v in measure_f32(c.measure() for c in test_shade_sh.tolerance_cases().values()).items()})
