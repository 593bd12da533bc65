"""The restatement `dirt_amd.shading.shadow_visibility` (and its torch form `dirt_amd.lighting.shadow_visibility`) is checked
against: the specification of DESIGN.md §7h in float64 with autograd, written from the other end -- the visibility as the MEAN
OF kernel^2 BILINEAR BLENDS of the comparison at the texel offsets -h .. h, each blend in its difference form, not as one window
of (kernel + 1)^2 weighted texels -- so that it shares neither code nor the window's weights with `dirt_amd.lighting`
(tests/test_shadow.py holds the two against each other).

The L1 mass of an element is the sum of the absolute values of the terms it is added up from.  out = 1 - m (1 - v) has the
terms 1, m and m v.  The autograd path is cut at the clip-space point, as (x / w, y / w, z): the gradients of these three, of
the maps and of the mask are taken by autograd; the mass of d (x / w) and d (y / w) is the gradient of `vm`, v with every
difference of two comparisons written as their sum (in a lit region the gradient is an exact zero and its mass is not: the
terms are there and cancel); the maps', the mask's and z's terms all have the sign of m grad_out, so their mass is their
absolute value, taken with |grad_out|.  From there by hand: d clip = (d (x / w) / w, d (y / w) / w, d z, -(d (x / w) x / w +
d (y / w) y / w) / w), d matrices = [q, 1]^T d clip and d q = d clip M^T, sums of products whose masses are the same sums of
the absolute values; d n's is d q's through the absolute Jacobian of the normalisation.  An element whose mass is zero must be
exact.  `flat` marks the pixels whose every window holds one comparison only (lit, or in the umbra): the kernel owes them an
exact zero too, which tests/test_shadow.py asks for by itself.

The float32 torch form run on the same inputs is what users had before the kernel; its worst |f32 - ref64| / mass per kind of
result sets the tolerance (`measure_f32`):

    python -m tests.shadow_reference      # prints the float32 figures the F32 table of tests/test_shadow.py restates
"""
import numpy as np
import torch

from tests.shade_reference import worst_ratio

KINDS = ('out', 'd_positions', 'd_normals', 'd_mask', 'd_maps', 'd_matrices')
OFF_KINKS = 1.e-3     # random pixels keep this far from every kink (`kink_distance`)


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)).to(dtype)


def _smooth(t):
    u = t.clamp(0., 1.)
    return u * u * (3. - 2. * u)


def _visibility(nx, ny, d, front, Z, kernel, bias, softness):
    """One light: the points' x / w, y / w and clip z [N] each, front [N] (w > 0), Z [Hs, Ws] -> (v [N]; vm [N]: the L1 mass of
    v's terms that carry a gradient to the fractions -- every difference of comparisons a sum, the comparisons constants --, so
    that d vm / d (x / w) and d vm / d (y / w) are the masses of d v / d (x / w), d v / d (y / w); the distance [N] of each point
    from the nearest kink: a lattice line of row or col (where a window edge crosses the map's border too), t at 0 or 1 at a
    texel of the window; flat [N]: every comparison of the window is the same, or there is no window)"""
    Hs, Ws = Z.shape
    h = (kernel - 1) // 2
    col = (nx + 1.) * Ws / 2. - 0.5
    row = (1. - ny) * Hs / 2. - 0.5
    fr0, fc0 = torch.floor(row.detach()), torch.floor(col.detach())
    # the window's rows fr0 - h .. fr0 + h + 1 against the map's 0 .. Hs - 1
    on = front & (fr0 + h + 1 >= 0) & (fr0 - h <= Hs - 1) & (fc0 + h + 1 >= 0) & (fc0 - h <= Ws - 1)
    zero = torch.zeros_like(row)
    row, col, fr0, fc0 = (torch.where(on, a, zero) for a in (row, col, fr0, fc0))
    fr, fc = row - fr0, col - fc0
    r_lo, c_lo = fr0.long(), fc0.long()
    kink = torch.minimum(torch.minimum(fr, 1. - fr), torch.minimum(fc, 1. - fc)).detach()
    kink = torch.where(on, kink, torch.full_like(kink, float('inf')))

    def S(r, c):
        inside = (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws)
        t = (Z[r.clamp(0, Hs - 1), c.clamp(0, Ws - 1)] - d + bias) / softness + 0.5
        edge = torch.minimum(t.abs(), (t - 1.).abs()).detach()
        return torch.where(inside, _smooth(t), torch.ones_like(t)), torch.where(inside & on, edge, torch.full_like(edge, float('inf')))

    total, total_m = torch.zeros_like(row), torch.zeros_like(row)
    lowest, highest = torch.full_like(row, float('inf')), torch.full_like(row, -float('inf'))
    for i in range(-h, h + 1):
        for j in range(-h, h + 1):
            (s00, k00), (s01, k01), (s10, k10), (s11, k11) = (S(r_lo + i + a, c_lo + j + b) for a in (0, 1) for b in (0, 1))
            total = total + (s00 + fr * (s10 - s00) + fc * (s01 - s00) + fr * fc * ((s11 - s10) - (s01 - s00)))
            c00, c01, c10, c11 = (s.detach() for s in (s00, s01, s10, s11))
            total_m = total_m + (fr * (c10 + c00) + fc * (c01 + c00) + (fr * fc.detach() + fr.detach() * fc) * ((c11 + c10) + (c01 + c00)))
            for k in (k00, k01, k10, k11):
                kink = torch.minimum(kink, k)
            for s in (c00, c01, c10, c11):
                lowest, highest = torch.minimum(lowest, s), torch.maximum(highest, s)
    v = total / float(kernel * kernel)
    return torch.where(on, v, torch.ones_like(v)), torch.where(on, total_m / float(kernel * kernel), zero), kink, ~on | (lowest == highest)


def compose(gbuffer, maps, matrices, layout, kernel=3, bias=0., softness=1., normal_offset=0., grad_out=None, dtype=torch.float64,
            masses=True):
    """One scene: gbuffer [N, Cg], maps [L, Hs, Ws], matrices [L, 4, 4] (float32 values), layout = (positions, normals or None,
    mask or None: channel indices) -> dict: out [N, L], kink [N], flat [N] (every light's window holds one comparison only: the
    point and the normal get no gradient); with grad_out [N, L] also d_gbuffer [N, Cg], d_maps, d_matrices; with masses mass_out
    and mass_<each of those>."""
    op, on, om = layout
    g = _t(gbuffer, dtype)
    N, Cg = g.shape
    p = g[:, op:op + 3].clone().requires_grad_(True)
    use_n = normal_offset != 0.
    n = g[:, on:on + 3].clone().requires_grad_(True) if use_n else None
    m = (g[:, om].clone() if om is not None else torch.ones(N, dtype=dtype)).requires_grad_(True)
    Z = _t(maps, dtype).requires_grad_(True)
    M = _t(matrices, dtype)
    L = Z.shape[0]
    q = p
    if use_n:
        length = torch.linalg.vector_norm(n, dim=-1, keepdim=True)      # (its gradient at a zero vector is 0; sqrt's would be inf)
        q = p + normal_offset * (n / length.clamp_min(1.e-12))
    q4 = torch.cat([q, torch.ones_like(q[:, :1])], 1)
    # the cut: behind it the clip-space point is a constant, and its gradient is chained on by hand
    x, y, z, w = torch.einsum('ni,lij->lnj', q4, M).detach().unbind(-1)
    front = w > 0
    ws = torch.where(front, w, torch.ones_like(w))
    nx, ny, d = ((x / ws).requires_grad_(True), (y / ws).requires_grad_(True), z.clone().requires_grad_(True))
    vs, vms, kinks, flats = zip(*(_visibility(nx[l], ny[l], d[l], front[l], Z[l], kernel, bias, softness) for l in range(L)))
    v, vm = torch.stack(vs, 1), torch.stack(vms, 1)
    out = 1. - m[:, None] * (1. - v)
    near_zero_w = torch.where(torch.isnan(w), torch.zeros_like(w), w.abs()).min(0).values
    res = {'out': out.detach().numpy(), 'kink': torch.minimum(torch.stack(kinks, 1).min(1).values, near_zero_w).numpy(),
           'flat': torch.stack(flats, 1).all(1).numpy()}
    if masses:
        res['mass_out'] = (1. + m.detach().abs()[:, None] * (1. + v.detach())).numpy()
    if grad_out is None:
        return res
    go = _t(grad_out, dtype)
    g_nx, g_ny, g_d, dZ, dm = torch.autograd.grad((out * go).sum(), [nx, ny, d, Z, m], retain_graph=True)
    nxd, nyd = nx.detach(), ny.detach()
    # x / w, y / w -> x, y, w, for the points in front of the light (the others have no gradient: theirs are zeros already)
    dclip = torch.stack([g_nx / ws, g_ny / ws, g_d, -(g_nx * nxd + g_ny * nyd) / ws], -1)
    q4d = q4.detach()
    dM = torch.einsum('ni,lnj->lij', q4d, dclip)
    dq = torch.einsum('lnj,lij->ni', dclip, M)[:, :3]
    dn = torch.autograd.grad(q, n, grad_outputs=dq)[0] if use_n else None

    def rows(d_p, d_n, d_m):
        out_rows = torch.zeros(N, Cg, dtype=dtype)
        out_rows[:, op:op + 3] = d_p
        if use_n:
            out_rows[:, on:on + 3] = d_n
        if om is not None:
            out_rows[:, om] = d_m
        return out_rows.numpy()

    res.update(d_gbuffer=rows(dq, dn, dm), d_maps=dZ.numpy(), d_matrices=dM.numpy())
    if not masses:
        return res
    weight = (m.detach().abs()[:, None] * go.abs())
    m_nx, m_ny = (t.abs() for t in torch.autograd.grad((vm * weight).sum(), [nx, ny]))      # (vm's only paths: row, col)
    mass_dclip = torch.stack([m_nx / ws.abs(), m_ny / ws.abs(), g_d.abs(), (m_nx * nxd.abs() + m_ny * nyd.abs()) / ws.abs()], -1)
    mass_dq = torch.einsum('lnj,lij->ni', mass_dclip, M.abs())[:, :3]
    mass_dn = None
    if use_n:
        nd = n.detach()
        length = torch.sqrt((nd * nd).sum(-1, keepdim=True))
        unit = nd / length.clamp_min(1.e-12)
        eye = torch.eye(3, dtype=dtype)
        jac = torch.where((length >= 1.e-12)[:, :, None], (eye - unit[:, :, None] * unit[:, None, :]) / length.clamp_min(1.e-12)[:, :, None],
                          eye.expand(N, 3, 3) * 1.e12) * abs(normal_offset)
        mass_dn = torch.einsum('nij,nj->ni', jac.abs(), mass_dq)
    mass_dm = (go.abs() * (1. + v.detach())).sum(1)
    mass_dZ = torch.autograd.grad((out * go.abs()).sum(), Z)[0].abs()
    res.update(mass_d_gbuffer=rows(mass_dq, mass_dn, mass_dm), mass_d_maps=mass_dZ.numpy(),
               mass_d_matrices=torch.einsum('ni,lnj->lij', q4d.abs(), mass_dclip).numpy())
    return res


def torch_form(gbuffer, maps, matrices, layout, kernel=3, bias=0., softness=1., normal_offset=0., grad_out=None, dtype=torch.float32):
    """the route users had: `lighting.shadow_visibility` on slices of the G-buffer, on the CPU in `dtype` -> the keys of `compose`"""
    from dirt_amd import lighting
    op, on, om = layout
    g = _t(gbuffer, dtype).requires_grad_(True)
    Z, M = _t(maps, dtype).requires_grad_(True), _t(matrices, dtype).requires_grad_(True)
    out = lighting.shadow_visibility(g[:, op:op + 3], g[:, on:on + 3] if normal_offset != 0. else None, Z, M,
                                     mask=g[:, om] if om is not None else None, kernel=kernel, bias=bias, softness=softness,
                                     normal_offset=normal_offset)
    res = {'out': out.detach().numpy()}
    if grad_out is not None:
        out.backward(_t(grad_out, dtype))
        zero = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(tuple(x.shape))   # noqa: E731
        res.update(d_gbuffer=zero(g), d_maps=zero(Z), d_matrices=zero(M))
    return res


def ratios(got, ref, layout, normal_offset=0.):
    """The worst |got - ref| / mass per kind of result (KINDS; d gbuffer by attribute); got: dict with out, d_gbuffer, d_maps,
    d_matrices (entries that are missing or None are skipped), ref: `compose(..., masses=True)`."""
    op, on, om = layout
    as64 = lambda x: np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)   # noqa: E731
    worst = {}
    for kind in ('out', 'd_maps', 'd_matrices'):
        if got.get(kind) is not None and kind in ref:
            worst[kind] = worst_ratio(as64(got[kind]).reshape(ref[kind].shape), ref[kind], ref['mass_' + kind])
    if got.get('d_gbuffer') is not None and 'd_gbuffer' in ref:
        dg = as64(got['d_gbuffer']).reshape(ref['d_gbuffer'].shape)
        spans = [('d_positions', slice(op, op + 3))]
        if normal_offset != 0.:
            spans.append(('d_normals', slice(on, on + 3)))
        if om is not None:
            spans.append(('d_mask', slice(om, om + 1)))
        for kind, s in spans:
            worst[kind] = worst_ratio(dg[:, s], ref['d_gbuffer'][:, s], ref['mass_d_gbuffer'][:, s])
    return worst


def exact_where_massless(got, ref):
    """Whether every element of d_gbuffer, d_maps and d_matrices whose mass is zero equals the reference (a zero) exactly"""
    for kind in ('d_gbuffer', 'd_maps', 'd_matrices'):
        if got.get(kind) is None or kind not in ref:
            continue
        x = np.asarray(got[kind].detach().cpu() if isinstance(got[kind], torch.Tensor) else got[kind], dtype=np.float64).reshape(ref[kind].shape)
        zero = ref['mass_' + kind] == 0
        if not np.array_equal(x[zero], ref[kind][zero]):
            return False
    return True


def measure_f32(cases):
    """cases: iterable of (positional arguments, keyword arguments) of `compose` -> the worst |f32 - ref64| / mass of the float32
    torch form per kind of result"""
    worst = dict.fromkeys(KINDS, 0.)
    for args, kw in cases:
        ref = compose(*args, **kw)
        r32 = torch_form(*args, dtype=torch.float32, **kw)
        for k, x in ratios(r32, ref, args[3], kw.get('normal_offset', 0.)).items():
            assert x == x, (k, 'a NaN')
            worst[k] = max(worst[k], x)
    return worst


# ---- inputs off the kinks

def light_matrix(rng, perspective):
    """A light above the scene, looking down -z of its own frame after a small random rotation: world -> clip, row vectors,
    float32.  The scene's box |x|, |y| <= 1.3, |z| <= 1 overhangs the map on every side."""
    from dirt_amd import matrices
    rot = matrices.rodrigues(torch.as_tensor(rng.uniform(-0.25, 0.25, 3), dtype=torch.float64))
    view = matrices.compose(rot, matrices.translation(torch.tensor([0.1, -0.05, -3.], dtype=torch.float64)))
    proj = matrices.perspective_projection(torch.tensor(1., dtype=torch.float64), 6., 0.4, 1.) if perspective \
        else matrices.orthographic_projection(torch.tensor(1., dtype=torch.float64), 6., 1.1, 1.)
    return matrices.compose(view, proj).numpy().astype(np.float32)


def depth_range(perspective):
    """the clip z of the scene's box under `light_matrix`, roughly: what the maps' noise spans"""
    return (0.2, 3.4) if perspective else (-0.7, 0.3)


def random_scene(rng, lights, hs, ws):
    """(maps [L, hs, ws] of noise over each light's depth range, matrices [L, 4, 4], softness: a third of the narrowest range);
    the even lights are orthographic, the odd ones perspective"""
    mats = np.stack([light_matrix(rng, l % 2 == 1) for l in range(lights)])
    maps = np.stack([rng.uniform(*depth_range(l % 2 == 1), (hs, ws)) for l in range(lights)]).astype(np.float32)
    return maps, mats


def random_pixels(rng, n, cg, layout, covered=0.8, behind=0.05):
    """A G-buffer [n, cg] of noise with positions in the scene's box (a share `behind`: far above it, behind every light),
    normals standard-normal vectors (every second pixel: of unit length, every seventh: zero) and a mask of 0 / 1 (a tenth: a
    fraction, as an antialiased edge leaves it)"""
    op, on, om = layout
    g = rng.standard_normal((n, cg)).astype(np.float32)
    pos = rng.uniform(-1., 1., (n, 3)) * np.array([1.3, 1.3, 1.])
    far = rng.uniform(0., 1., n) < behind
    pos[far, 2] += 5.
    g[:, op:op + 3] = pos
    if on is not None:
        nn = rng.standard_normal((n, 3))
        nn[::2] /= np.linalg.norm(nn[::2], axis=-1, keepdims=True)
        nn[::7] = 0.
        g[:, on:on + 3] = nn
    if om is not None:
        mask = (rng.uniform(0., 1., n) < covered).astype(np.float64)
        frac = rng.uniform(0., 1., n) < 0.1
        mask[frac] = rng.uniform(0.1, 0.9, int(frac.sum()))
        g[:, om] = mask
    return g


def draw_off_kinks(rng, n, cg, layout, maps, mats, kw, max_rejected=0.5):
    """Random pixels that keep OFF_KINKS from every kink, judged by the float64 values alone: draw, reject, redraw the rejected
    pixels.  -> (gbuffer [n, cg], the share rejected from the first draw)"""
    g = random_pixels(rng, n, cg, layout)
    share = None
    for _ in range(40):
        bad = compose(g, maps, mats, layout, masses=False, **kw)['kink'] < OFF_KINKS
        if share is None:
            share = float(bad.mean())
            assert share < max_rejected, 'share of rejected pixels %.3f' % share
        if not bad.any():
            return g, share
        g[bad] = random_pixels(rng, int(bad.sum()), cg, layout)
    raise AssertionError('could not draw pixels off the kinks')


if __name__ == '__main__':
    from tests import test_shadow
    print({k: '%.3e' % v for k, v in measure_f32(test_shadow.tolerance_cases()).items()})
