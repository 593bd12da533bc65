"""The restatement `dirt_amd.shading.environment_background` (and its torch form `dirt_amd.lighting.environment_background`)
is checked against: the specification of DESIGN.md §7i in numpy float64, written from the other end -- the rays as two
homogeneous products [nx, ny, z, 1] @ M, the face as a table of three basis vectors (sc, tc and the major axis are dot
products with them, and the direction gradient is their weighted sum), the bilinear blend in its difference form, and every
gradient by hand -- so that it shares neither code nor order of operations with `dirt_amd.lighting`.

The L1 mass of an element is the sum of the absolute values of the terms it is added up from.  The blend weights are not
negative, so with Eabs the look-up of |environment|: out_j = (1 - m) I_j E_j has the mass |1 - m| |I_j| Eabs_j; d I_j = sum (1 -
m) E_j g_j the mass sum |1 - m| Eabs_j |g_j|; d m = -sum_j I_j E_j g_j the mass sum_j |I_j| Eabs_j |g_j|; a texel of d environment
the sum of |(1 - m) I_j g_j| times its weights.  The derivative of a blend by its fraction is a sum of differences of texels, its
mass the same sum of their absolute values; from there the masses follow the chain rule with every factor's absolute value:
through (sc / a, tc / a), the face's basis, the two divisions by h.w and the sixteen sums
d M = sum [nx, ny, 0, 1]^T g0 + [nx, ny, -1, 1]^T gm.  An element whose mass is zero must be exact.

The float32 torch form run on the same inputs is what a user had before the kernel; its worst |f32 - ref64| / mass per kind
of result sets the tolerance (`measure_f32`):

    python -m tests.background_reference      # prints the float32 figures the F32 table of tests/test_background.py restates
"""
import numpy as np
import torch

from tests.shade_reference import worst_ratio

KINDS = ('out', 'd_environment', 'd_matrix', 'd_intensity', 'd_mask')
OFF_KINKS = 1.e-3       # pixels closer than this to a kink are not compared (`kink` below)
LAMBDA_MARGIN = 0.05    # ... and those whose footprint lambda lies this close to an integer level

# per face +X, -X, +Y, -Y, +Z, -Z: the vectors whose dot products with a direction are sc, tc and the major component's magnitude
SC = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], dtype=np.float64)
TC = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], dtype=np.float64)
MA = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def level_count(n, max_level=None):
    levels = 1
    while n % 2 == 0 and (max_level is None or levels <= max_level):
        n, levels = n // 2, levels + 1
    return levels


def box_levels(cube, max_level=None):
    """[level 0 = cube [6, N, N, 3], level 1, ...] in float32, each the 2 x 2 means ((t00 + t01) + (t10 + t11)) * 0.25 of the one
    below: the pyramid the library builds of a cube"""
    t = np.asarray(cube, np.float32)
    out = [t]
    for _ in range(1, level_count(t.shape[1], max_level)):
        t = (((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])) * np.float32(0.25)).astype(np.float32)
        out.append(t)
    return out


def collapse(level_grads):
    """The gradients of a box pyramid's levels -> the gradient of the cube they were built of (masses likewise: every factor is
    positive): a texel of level k is the mean of 4^k texels of level 0"""
    total = np.zeros_like(level_grads[0])
    for k, g in enumerate(level_grads):
        total += np.repeat(np.repeat(g, 2 ** k, axis=1), 2 ** k, axis=2) / 4. ** k
    return total


def pack(levels):
    """levels [6, n_k, n_k, 3] -> [6, floats]: `CubePyramid.packed`'s layout"""
    return np.concatenate([np.asarray(lv).reshape(6, -1) for lv in levels], axis=1)


def rays(M, H, W):
    """-> nx, ny [H, W], h0, hm [H, W, 4]: the homogeneous world points of the pixel centres on clip z = 0 and z = -1"""
    M = np.asarray(M, np.float64)
    nx = np.broadcast_to((2. * (np.arange(W) + 0.5) / W - 1.)[None, :], (H, W))
    ny = np.broadcast_to((1. - 2. * (np.arange(H) + 0.5) / H)[:, None], (H, W))
    one = np.ones((H, W))
    p0, pm = np.stack([nx, ny, 0. * one, one], -1), np.stack([nx, ny, -one, one], -1)
    return nx, ny, p0 @ M, pm @ M, p0, pm


class _Level:
    """The bilinear (or nearest) look-up of one level [6, n, n, 3] at face coordinates (s, t) of the valid pixels"""

    def __init__(self, level, face, s, t, nearest):
        self.lv = np.asarray(level, np.float64)
        self.n = n = self.lv.shape[1]
        self.face, self.nearest = face, nearest
        self.x = [(t + 1.) / 2. * n - 0.5, (s + 1.) / 2. * n - 0.5]            # row, column before the clamp
        self.inside = [(x >= 0) & (x <= n - 1) for x in self.x]
        xc = [np.clip(x, 0., n - 1.) for x in self.x]
        if nearest:
            i = [np.clip(np.floor(x + 0.5).astype(np.int64), 0, n - 1) for x in xc]
            self.idx = [(i[0], i[1])]
            self.wts = [np.ones_like(s)]
            self.fr = self.fc = np.zeros_like(s)
        else:
            lo = [np.clip(np.floor(x).astype(np.int64), 0, n - 1) for x in xc]
            hi = [np.minimum(l + 1, n - 1) for l in lo]
            self.fr, self.fc = xc[0] - np.floor(xc[0]), xc[1] - np.floor(xc[1])
            self.idx = [(lo[0], lo[1]), (lo[0], hi[1]), (hi[0], lo[1]), (hi[0], hi[1])]     # tl, tr, bl, br
            self.wts = [(1. - self.fc) * (1. - self.fr), self.fc * (1. - self.fr), (1. - self.fc) * self.fr, self.fc * self.fr]
        self.box = (self.idx[0][0], self.idx[-1][0], self.idx[0][1], self.idx[-1][1])      # r0, r1, c0, c1

    def texels(self, lv=None):
        lv = self.lv if lv is None else lv
        return [lv[self.face, r, c] for r, c in self.idx]

    def value(self, absolute=False):
        T = self.texels(np.abs(self.lv) if absolute else None)
        if self.nearest:
            return T[0]
        tl, tr, bl, br = T
        if absolute:
            return sum(w[:, None] * x for w, x in zip(self.wts, T))
        fr, fc = self.fr[:, None], self.fc[:, None]
        return tl + fc * (tr - tl) + fr * (bl - tl) + fr * fc * ((br - bl) - (tr - tl))

    def slopes(self, absolute=False):
        """d value / d s and d value / d t per channel (their masses with `absolute`): zero where the index is clamped"""
        if self.nearest:
            z = np.zeros((len(self.face), 3))
            return z, z
        tl, tr, bl, br = self.texels(np.abs(self.lv) if absolute else None)
        fr, fc = self.fr[:, None], self.fc[:, None]
        sign = 1. if absolute else -1.
        d_fc = (tr + sign * tl) * (1. - fr) + (br + sign * bl) * fr
        d_fr = (bl + sign * tl) * (1. - fc) + (br + sign * tr) * fc
        half = self.n / 2.
        return d_fc * (self.inside[1] * half)[:, None], d_fr * (self.inside[0] * half)[:, None]

    def scatter(self, grads, weight):
        """grads [6, n, n, 3] += weight [pixels, 3] times the taps' weights"""
        for (r, c), w in zip(self.idx, self.wts):
            np.add.at(grads, (self.face, r, c), weight * w[:, None])

    def kink(self):
        """the distance of the index from a lattice line or a clamp end (nearest: from the middle between two texels)"""
        dist = np.full(len(self.face), np.inf)
        for x, inside in zip(self.x, self.inside):
            frac = x - np.floor(x)
            at = np.abs(frac - 0.5) if self.nearest else np.minimum(frac, 1. - frac)
            ends = np.minimum(np.abs(x), np.abs(x - (self.n - 1)))
            dist = np.minimum(dist, np.where(inside, at, np.inf) if self.nearest else np.where(inside, np.minimum(at, ends), ends))
        return dist

    def clamped(self):
        return ~(self.inside[0] & self.inside[1])


def compose(levels, M, size, mask=None, intensity=(1., 1., 1.), filter='bilinear', lod=None, lod_bias=0., grad_out=None):
    """One scene.  levels: the environment's levels [6, n_k, n_k, 3] (float32 values; one level unless filter is 'trilinear'),
    M [4, 4], size (H, W), mask [H, W] or None, intensity [3] -> dict: out [H, W, 3], valid, face (-1: not valid), lam (before
    the clamp), level (the lower touched level), two (a second level carries weight), clamped, kink [H, W], box0 / box1 (r0, r1,
    c0, c1 of the taps at the touched levels, [H, W] each), mass_out; with grad_out [H, W, 3] also d_levels (a list like
    `levels`), d_matrix [4, 4], d_intensity [3], d_mask [H, W] and mass_<each>."""
    H, W = size
    levels = [np.asarray(lv, np.float64) for lv in levels]
    L, N = len(levels), levels[0].shape[1]
    I = np.asarray(intensity, np.float64)
    m = np.zeros((H, W)) if mask is None else np.asarray(mask, np.float64)
    w = 1. - m
    nx, ny, h0, hm, p0, pm = rays(M, H, W)
    with np.errstate(all='ignore'):
        end, start = h0[..., :3] / h0[..., 3:], hm[..., :3] / hm[..., 3:]
        d = end - start
        valid = np.isfinite(d).all(-1) & (np.abs(d).max(-1) > 0) & (w != 0)
    v = np.nonzero(valid.reshape(-1))[0]
    dv, endv, startv = d.reshape(-1, 3)[v], end.reshape(-1, 3)[v], start.reshape(-1, 3)[v]
    h0w, hmw = h0[..., 3].reshape(-1)[v], hm[..., 3].reshape(-1)[v]
    ad = np.abs(dv)
    major = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    face = 2 * major + (dv[np.arange(len(v)), major] <= 0)
    a = np.einsum('ij,ij->i', dv, MA[face])
    s, t = np.einsum('ij,ij->i', dv, SC[face]) / a, np.einsum('ij,ij->i', dv, TC[face]) / a
    # the level of detail
    lam = np.zeros(len(v))
    if filter == 'trilinear':
        if lod is None:
            n2 = []
            for axis, n in ((0, W), (1, H)):
                row = np.asarray(M, np.float64)[axis]
                dd = (2. / n) * ((row[:3] - endv * row[3]) / h0w[:, None] - (row[:3] - startv * row[3]) / hmw[:, None])
                dma = np.einsum('ij,ij->i', dd, MA[face])
                ds = (np.einsum('ij,ij->i', dd, SC[face]) - s * dma) / a
                dt = (np.einsum('ij,ij->i', dd, TC[face]) - t * dma) / a
                n2.append(ds * ds + dt * dt)
            with np.errstate(divide='ignore'):
                lam = np.log2(N / 2. * np.sqrt(np.maximum(n2[0], n2[1]))) + float(np.float32(lod_bias))
        else:
            lam = np.full(len(v), float(np.float32(lod) + np.float32(lod_bias)))
    lam_c = np.clip(lam, 0., L - 1.)
    l0 = np.floor(lam_c).astype(np.int64)
    f = lam_c - l0
    two = f != 0
    nearest = filter == 'nearest'
    # the look-ups, level by level (a pixel touches level l0 and, where f != 0, l0 + 1)
    E, Eabs = np.zeros((len(v), 3)), np.zeros((len(v), 3))
    slope_s, slope_t, mass_s, mass_t = (np.zeros((len(v), 3)) for _ in range(4))
    kink = np.full(len(v), np.inf)
    clamped = np.zeros(len(v), bool)
    boxes = np.full((2, 4, len(v)), -1, np.int64)
    looks = []
    for k in range(L):
        for second in (0, 1):
            sel = np.nonzero((l0 + second == k) & (two | (second == 0)))[0]
            if not len(sel):
                continue
            lk = _Level(levels[k], face[sel], s[sel], t[sel], nearest)
            wk = (f[sel] if second else 1. - f[sel])[:, None]
            E[sel] += wk * lk.value()
            Eabs[sel] += wk * lk.value(True)
            for tot, part in zip((slope_s, slope_t), lk.slopes()):
                tot[sel] += wk * part
            for tot, part in zip((mass_s, mass_t), lk.slopes(True)):
                tot[sel] += wk * part
            kink[sel] = np.minimum(kink[sel], lk.kink())
            clamped[sel] |= lk.clamped()
            boxes[second][:, sel] = np.stack(lk.box)
            looks.append((k, sel, lk, wk))
    sorted_ad = np.sort(ad, axis=1)
    kink = np.minimum(kink, (sorted_ad[:, 2] - sorted_ad[:, 1]) / sorted_ad[:, 2])                     # a face boundary
    kink = np.minimum(kink, np.minimum(np.abs(h0w), np.abs(hmw)))                                       # h.w = 0
    if filter == 'trilinear' and lod is None and L > 1:
        near = np.abs(lam - np.clip(np.round(lam), 0, L - 1))
        kink = np.minimum(kink, near * (OFF_KINKS / LAMBDA_MARGIN))

    def image(x, fill=0.):
        full = np.full((H * W,) + x.shape[1:], fill, dtype=x.dtype)
        full[v] = x
        return full.reshape((H, W) + x.shape[1:])

    wv = w.reshape(-1)[v][:, None]
    res = {'out': image(wv * I * E), 'mass_out': image(np.abs(wv) * np.abs(I) * Eabs), 'valid': valid, 'face': image(face, -1),
           'lam': image(lam), 'level': image(l0, -1), 'two': image(two), 'clamped': image(clamped), 'kink': image(kink, np.inf),
           'direction': np.where(valid[..., None], d, 0.), 'box0': [image(b, -1) for b in boxes[0]], 'box1': [image(b, -1) for b in boxes[1]]}
    if grad_out is None:
        return res
    g = np.asarray(grad_out, np.float64).reshape(-1, 3)[v]
    res['d_intensity'], res['mass_d_intensity'] = (wv * E * g).sum(0), (np.abs(wv) * Eabs * np.abs(g)).sum(0)
    res['d_mask'], res['mass_d_mask'] = image(-(I * E * g).sum(1)), image((np.abs(I) * Eabs * np.abs(g)).sum(1))
    gE = wv * I * g
    d_levels, m_levels = [np.zeros_like(lv) for lv in levels], [np.zeros_like(lv) for lv in levels]
    for k, sel, lk, wk in looks:
        lk.scatter(d_levels[k], wk * gE[sel])
        lk.scatter(m_levels[k], wk * np.abs(gE[sel]))
    res['d_levels'], res['mass_d_levels'] = d_levels, m_levels
    # the direction: through (sc / a, tc / a) and the face's basis
    gs, gt = (gE * slope_s).sum(1), (gE * slope_t).sum(1)
    ms, mt = (np.abs(gE) * mass_s).sum(1), (np.abs(gE) * mass_t).sum(1)
    g_a, m_a = -(gs * s + gt * t) / a, (ms * np.abs(s) + mt * np.abs(t)) / a
    gd = (gs / a)[:, None] * SC[face] + (gt / a)[:, None] * TC[face] + g_a[:, None] * MA[face]
    md = (ms / a)[:, None] * np.abs(SC[face]) + (mt / a)[:, None] * np.abs(TC[face]) + m_a[:, None] * np.abs(MA[face])
    # d = end - start, end = h0.xyz / h0.w, start = hm.xyz / hm.w
    g0 = np.concatenate([gd / h0w[:, None], -(gd * endv).sum(1, keepdims=True) / h0w[:, None]], 1)
    gm = np.concatenate([-gd / hmw[:, None], (gd * startv).sum(1, keepdims=True) / hmw[:, None]], 1)
    m0 = np.concatenate([md, (md * np.abs(endv)).sum(1, keepdims=True)], 1) / np.abs(h0w)[:, None]
    mm = np.concatenate([md, (md * np.abs(startv)).sum(1, keepdims=True)], 1) / np.abs(hmw)[:, None]
    p0v, pmv = p0.reshape(-1, 4)[v], pm.reshape(-1, 4)[v]
    res['d_matrix'] = p0v.T @ g0 + pmv.T @ gm                      # the sixteen sums
    res['mass_d_matrix'] = np.abs(p0v).T @ m0 + np.abs(pmv).T @ mm
    return res


PER_PIXEL = ('out', 'mass_out', 'valid', 'face', 'lam', 'level', 'two', 'clamped', 'kink', 'direction', 'd_mask', 'mass_d_mask')


def compose_batch(levels, M, size, mask=None, intensity=(1., 1., 1.), grad_out=None, **kw):
    """`compose` for a batch: M [B, 4, 4], mask [B, H, W], intensity [B, 3], whichever has the leading B (the others are shared
    by the scenes), grad_out [B, H, W, 3] -> the per-pixel results stacked [B, ...], d_matrix / d_intensity / d_mask stacked for a
    per-scene operand and summed over the scenes for a shared one, d_levels summed.  Without a leading B anywhere: `compose`."""
    M, I = np.asarray(M), np.asarray(intensity)
    batched = [x.shape[0] for x, rank in ((M, 3), (I, 2)) if x.ndim == rank] + ([np.shape(mask)[0]] if mask is not None and np.ndim(mask) == 3 else [])
    if not batched:
        return compose(levels, M, size, mask, I, grad_out=grad_out, **kw)
    assert len(set(batched)) == 1
    pick = lambda x, rank, b: x if x is None or np.ndim(x) < rank else x[b]   # noqa: E731
    scenes = [compose(levels, pick(M, 3, b), size, pick(mask, 3, b), pick(I, 2, b), grad_out=None if grad_out is None else grad_out[b], **kw)
              for b in range(batched[0])]
    res = {k: np.stack([s[k] for s in scenes]) for k in PER_PIXEL if k in scenes[0]}
    res['box0'], res['box1'] = ([np.stack([s[key][i] for s in scenes]) for i in range(4)] for key in ('box0', 'box1'))
    if grad_out is None:
        return res
    for key, x, rank in (('d_matrix', M, 3), ('d_intensity', I, 2), ('d_mask', mask, 3)):
        for k in (key, 'mass_' + key):
            res[k] = np.stack([s[k] for s in scenes]) if x is not None and np.ndim(x) == rank else sum(s[k] for s in scenes)
    for k in ('d_levels', 'mass_d_levels'):
        res[k] = [sum(s[k][l] for s in scenes) for l in range(len(levels))]
    return res


def environment_grad(ref, operand):
    """(d environment, its mass) of `compose`'s result in the shape of the operand: 'cube' (the levels are the box pyramid of a
    cube: collapsed), 'packed' (a CubePyramid: [6, floats])"""
    if operand == 'cube':
        return collapse(ref['d_levels']), collapse(ref['mass_d_levels'])
    return pack(ref['d_levels']), pack(ref['mass_d_levels'])


def torch_form(levels, M, size, mask=None, intensity=(1., 1., 1.), filter='bilinear', lod=None, lod_bias=0., grad_out=None, operand='cube',
               dtype=torch.float32):
    """the route the specification names: `lighting.environment_background` on the CPU in `dtype` -> out, d_environment,
    d_matrix, d_intensity, d_mask.  operand 'cube': the environment is levels[0] and the form builds its own box pyramid;
    'packed': a CubePyramid of the levels"""
    from dirt_amd import lighting
    from dirt_amd.texture import CubePyramid
    as_t = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(dtype)   # noqa: E731
    if operand == 'cube':
        leaf = as_t(levels[0]).requires_grad_(True)
        env, kw = leaf, dict(max_level=len(levels) - 1) if filter == 'trilinear' else {}
    else:
        leaf = as_t(pack(levels)).requires_grad_(True)
        env, kw = CubePyramid(leaf, levels[0].shape[1], 3, len(levels)), {}
    Mt, It = as_t(M).requires_grad_(True), as_t(intensity).requires_grad_(True)
    mt = None if mask is None else as_t(mask).requires_grad_(True)
    if filter == 'trilinear':
        kw.update(lod=lod, lod_bias=lod_bias)
    out = lighting.environment_background(env, Mt, size, mask=mt, intensity=It, filter=filter, **kw)
    res = {'out': out.detach().numpy()}
    if grad_out is not None:
        out.backward(as_t(grad_out))
        zero = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(tuple(x.shape))   # noqa: E731
        res.update(d_environment=zero(leaf), d_matrix=zero(Mt), d_intensity=zero(It), d_mask=None if mt is None else zero(mt))
    return res


def ratios(got, ref, operand='cube', keep=None):
    """The worst |got - ref| / mass per kind of result (KINDS); got: dict (entries that are missing or None are skipped), ref:
    `compose`'s.  keep [H, W]: the pixels compared in the per-pixel kinds (default: those off the kinks)"""
    keep = ref['kink'] >= OFF_KINKS if keep is None else keep
    as64 = lambda x: np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)   # noqa: E731
    worst = {}
    if got.get('out') is not None:
        worst['out'] = worst_ratio(as64(got['out'])[keep], ref['out'][keep], ref['mass_out'][keep])
    for kind in ('d_matrix', 'd_intensity', 'd_mask'):      # (sums, a shared mask's over the scenes: the pixels on kinks add nothing to them)
        if got.get(kind) is not None and kind in ref:
            worst[kind] = worst_ratio(as64(got[kind]).reshape(ref[kind].shape), ref[kind], ref['mass_' + kind])
    if got.get('d_environment') is not None and 'd_levels' in ref:
        want, mass = environment_grad(ref, operand)
        worst['d_environment'] = worst_ratio(as64(got['d_environment']).reshape(want.shape), want, mass)
    return worst


def exact_where_massless(got, ref, operand='cube'):
    """Whether every element of the sums whose mass is zero equals the reference (a zero) exactly"""
    pairs = [(got.get(k), ref[k], ref['mass_' + k]) for k in ('d_matrix', 'd_intensity', 'd_mask') if got.get(k) is not None and k in ref]
    if got.get('d_environment') is not None and 'd_levels' in ref:
        pairs.append((got['d_environment'],) + environment_grad(ref, operand))
    for x, want, mass in pairs:
        x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(want.shape)
        if not np.array_equal(x[mass == 0], want[mass == 0]):
            return False
    return True


def measure_f32(cases):
    """cases: iterable of (positional arguments, keyword arguments, operand) of `compose_batch` with the pixels on kinks taken out of
    the sums (`off_kinks`) -> the worst |f32 - ref64| / mass of the float32 torch form per kind of result"""
    worst = dict.fromkeys(KINDS, 0.)
    for args, kw, operand in cases:
        ref = compose_batch(*args, **kw)
        r32 = torch_form(*args, operand=operand, dtype=torch.float32, **kw)
        for k, x in ratios(r32, ref, operand).items():
            assert x == x, (k, 'a NaN')
            worst[k] = max(worst[k], x)
    return worst


def off_kinks(args, kw):
    """grad_out with zeros at the pixels within OFF_KINKS of a kink, judged by the float64 values alone: a pixel on a kink then
    adds nothing to any sum, whichever side of the kink float32 puts it on.  -> (grad_out, the share of pixels taken out)"""
    ref = compose_batch(*args, **dict(kw, grad_out=None))
    bad = ref['valid'] & (ref['kink'] < OFF_KINKS)
    go = np.array(kw['grad_out'], np.float32)
    go[bad] = 0.
    return go, float(bad.mean())


if __name__ == '__main__':
    from tests import test_background
    print({k: '%.3e' % v for k, v in measure_f32(test_background.tolerance_cases()).items()})
