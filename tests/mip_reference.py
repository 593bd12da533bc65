"""numpy restatement of the trilinear (mipmapped) texture look-up -- TEST INFRASTRUCTURE: dirt_amd never imports it.

The specification is DESIGN.md §7 (and the header of dirt_amd/csrc/dirt_texture_mip.hip): a pyramid of 2 x 2 / 2 x 1 means,
the level-k index max((index_0 - (s - 1) / 2) / s, 0), a level of detail from the (u, v) footprint or given, and a blend
of the bilinear samples of two adjacent levels.  `sample` follows the kernels' float32 operations (dtype=np.float64 gives
the same expression in double precision, for finite differences); `grad` is the analytic gradient, accumulated in
float64, with the L1 mass of each element's terms."""
import numpy as np


def level_count(ht, wt, max_level=None):
    levels, h, w = 1, ht, wt
    while not (h == 1 and w == 1) and (h == 1 or h % 2 == 0) and (w == 1 or w % 2 == 0) and (max_level is None or levels <= max_level):
        h, w, levels = max(h // 2, 1), max(w // 2, 1), levels + 1
    return levels


def pyramid(texture, max_level=None, dtype=np.float32):
    """[level 0 = texture, level 1, ...] in float32: ((t00 + t01) + (t10 + t11)) * 0.25, or (a + b) * 0.5."""
    dt = dtype
    t = np.asarray(texture, dt)
    out = [t]
    for _ in range(1, level_count(t.shape[0], t.shape[1], max_level)):
        hr, hc = t.shape[0] > 1, t.shape[1] > 1
        if hr and hc:
            t = ((t[0::2, 0::2] + t[0::2, 1::2]) + (t[1::2, 0::2] + t[1::2, 1::2])) * dt(0.25)
        elif hr:
            t = (t[0::2] + t[1::2]) * dt(0.5)
        else:
            t = (t[:, 0::2] + t[:, 1::2]) * dt(0.5)
        out.append(t.astype(dt))
    return out


def _indices(uvs, ht, wt, mode, dt):
    uvs = np.asarray(uvs, dt)[..., ::-1]
    shape = np.array([ht, wt], dt)
    with np.errstate(invalid='ignore'):
        if mode == 'repeat':
            return ((uvs - np.floor(uvs)).astype(dt) * shape).astype(dt)
        if mode == 'clamp':
            return (np.clip(uvs, dt(0), dt(1)) * shape).astype(dt)
    raise NotImplementedError(mode)


def footprint_lod(uvs, ht, wt, mode='repeat', mask=None, lod_bias=0.0):
    """lambda (before the clamp) of every pixel of images uvs [..., H, W, 2], float32 as the kernels compute it."""
    uv = np.asarray(uvs, np.float32)
    H, W = uv.shape[-3], uv.shape[-2]
    valid = np.ones(uv.shape[:-1], bool) if mask is None else (np.asarray(mask) != 0)
    zero = np.zeros_like(uv)

    def diff(axis, n):
        fwd = np.concatenate([np.diff(uv, axis=axis), np.zeros_like(np.take(uv, [0], axis=axis))], axis=axis)   # uv(+1) - uv
        bwd = np.concatenate([np.zeros_like(np.take(uv, [0], axis=axis)), np.diff(uv, axis=axis)], axis=axis)   # uv - uv(-1)
        vax = axis + 1   # the pixel axis in `valid` ([..., H, W])
        v_next = np.concatenate([np.take(valid, np.arange(1, n), axis=vax), np.zeros_like(np.take(valid, [0], axis=vax))], axis=vax)
        v_prev = np.concatenate([np.zeros_like(np.take(valid, [0], axis=vax)), np.take(valid, np.arange(0, n - 1), axis=vax)], axis=vax)
        return np.where(v_next[..., None], fwd, np.where(v_prev[..., None], bwd, zero)).astype(np.float32)

    dx, dy = diff(-2, W), diff(-3, H)
    if mode == 'repeat':
        dx = (dx - np.rint(dx)).astype(np.float32)
        dy = (dy - np.rint(dy)).astype(np.float32)
    Wf, Hf = np.float32(wt), np.float32(ht)
    ax, bx, ay, by = dx[..., 0] * Wf, dx[..., 1] * Hf, dy[..., 0] * Wf, dy[..., 1] * Hf
    rx = np.sqrt(ax * ax + bx * bx).astype(np.float32)
    ry = np.sqrt(ay * ay + by * by).astype(np.float32)
    with np.errstate(divide='ignore'):
        lam = (np.log2(np.fmax(rx, ry)) + np.float32(lod_bias)).astype(np.float32)
    return np.where(valid, lam, np.float32(0)).astype(np.float32)


def _split(lam, levels, dt):
    top = dt(levels - 1)
    c = np.where(lam > 0, np.where(lam < top, lam, top), dt(0)).astype(dt)
    fl = np.floor(c)
    return fl.astype(np.int64), (c - fl).astype(dt)


def _level_index(idx0, n0, nk, dt):
    """-> (index at level k, d index_k / d index_0) per axis."""
    s = dt(n0 / nk)
    x = ((idx0 - (s - dt(1)) * dt(0.5)) / s).astype(dt)
    return np.where(x < 0, dt(0), x).astype(dt), np.where(x < 0, 0.0, 1.0 / np.asarray(s, np.float64))


def _taps(row, col, h, w, dt):
    """Taps and fractions of bilinear_taps (per look-up arrays h, w: the level's size)."""
    fr0, fc0 = np.floor(row), np.floor(col)
    fr, fc = (row - fr0).astype(dt), (col - fc0).astype(dt)
    with np.errstate(invalid='ignore'):
        r0 = np.where(fr0 >= 1, np.minimum(np.where(np.isfinite(fr0), fr0, 0), h), 0).astype(np.int64)
        c0 = np.where(fc0 >= 1, np.minimum(np.where(np.isfinite(fc0), fc0, 0), w), 0).astype(np.int64)
    r0, c0 = np.minimum(r0, h - 1), np.minimum(c0, w - 1)
    return r0, np.minimum(r0 + 1, h - 1), c0, np.minimum(c0 + 1, w - 1), fr, fc


class _Look:
    """Per look-up quantities of one level set: the level, taps, fractions and the index derivatives."""

    def __init__(self, pyr, lev, row0, col0, dt):
        ht, wt = pyr[0].shape[:2]
        self.lev = lev
        h = np.array([p.shape[0] for p in pyr])[lev]
        w = np.array([p.shape[1] for p in pyr])[lev]
        rk, dr = _level_index(row0, ht, h, dt)
        ck, dc = _level_index(col0, wt, w, dt)
        at0 = lev == 0
        self.row = np.where(at0, row0, rk).astype(dt); self.col = np.where(at0, col0, ck).astype(dt)
        self.drow = np.where(at0, 1.0, dr); self.dcol = np.where(at0, 1.0, dc)
        self.r0, self.r1, self.c0, self.c1, self.fr, self.fc = _taps(self.row, self.col, h, w, dt)
        self.w = w
        self.offs = np.cumsum([0] + [p.size for p in pyr])[lev]

    def flat(self, r, c, ct):   # flat texel indices into the packed pyramid [n, ct]
        return (self.offs + (r * self.w + c) * ct)[:, None] + np.arange(ct)[None, :]


def _lambda(uvs, ht, wt, mode, lod, lod_bias, mask):
    if lod is not None:
        return (np.asarray(lod, np.float32) + np.float32(lod_bias)).astype(np.float32)
    return footprint_lod(uvs, ht, wt, mode, mask, lod_bias)


def sample(texture, uvs, mode='repeat', lod=None, lod_bias=0.0, mask=None, max_level=None, dtype=np.float32, magnitude=False):
    """The trilinear look-up [..., C]; magnitude=True also returns the sum of the bilinear samples of |pyramid| at both
    levels (the value's scale)."""
    dt = dtype
    pyr = pyramid(texture, max_level, dt)
    ht, wt, ct = pyr[0].shape
    uv = np.asarray(uvs, dt)
    if lod is not None and dt is not np.float32:
        lam = (np.asarray(lod, dt) + dt(lod_bias)).reshape(-1)
    else:
        lam = _lambda(uv, ht, wt, mode, lod, lod_bias, mask).reshape(-1).astype(dt)
    idx = _indices(uv.reshape(-1, 2), ht, wt, mode, dt)
    lev, f = _split(lam, len(pyr), dt)
    packed = np.concatenate([p.reshape(-1) for p in pyr])
    one = dt(1)

    def bil(look, src):
        a, b = src[look.flat(look.r0, look.c0, ct)], src[look.flat(look.r0, look.c1, ct)]
        c, d = src[look.flat(look.r1, look.c0, ct)], src[look.flat(look.r1, look.c1, ct)]
        fr, fc = look.fr[:, None], look.fc[:, None]
        wr0, wc0 = one - fr, one - fc
        return ((((a * wc0) * wr0) + ((b * fc) * wr0)) + ((c * wc0) * fr)) + ((d * fc) * fr)

    l0 = _Look(pyr, lev, idx[:, 0], idx[:, 1], dt)
    l1 = _Look(pyr, np.minimum(lev + 1, len(pyr) - 1), idx[:, 0], idx[:, 1], dt)
    out_shape = uv.shape[:-1] + (ct,)
    res = []
    s0, s1 = bil(l0, packed), bil(l1, packed)
    fv = f[:, None]
    with np.errstate(invalid='ignore'):
        out = np.where(fv == 0, s0, (one - fv) * s0 + fv * s1).astype(dt)
    if not magnitude:
        return out.reshape(out_shape)
    # the magnitude of both levels' samples: the value's scale, and its sensitivity to the fraction f (a log2 one ulp apart)
    mag = bil(l0, np.abs(packed)).astype(np.float64) + bil(l1, np.abs(packed))
    return out.reshape(out_shape), mag.reshape(out_shape)


def collapse(grad_levels, factors_of):
    """float64 collapse of per-level gradients [levels] (each [H_k, W_k, C]) to level 0: acc = g_{L-1}; acc = g_k + acc * factor."""
    acc = grad_levels[-1]
    for k in range(len(grad_levels) - 2, -1, -1):
        h, w = grad_levels[k].shape[:2]
        up = acc
        if up.shape[0] != h:
            up = np.repeat(up, 2, axis=0)
        if up.shape[1] != w:
            up = np.repeat(up, 2, axis=1)
        acc = grad_levels[k] + up * factors_of(k)
    return acc


def grad(texture, uvs, grad_out, mode='repeat', lod=None, lod_bias=0.0, mask=None, max_level=None):
    """-> dict grad_texture, grad_uvs, grad_lod (float64) and mass_texture, mass_uvs, mass_lod (their terms' L1 mass)."""
    pyr = pyramid(texture, max_level)
    pyr64 = [p.astype(np.float64) for p in pyr]
    L = len(pyr)
    ht, wt, ct = pyr[0].shape
    uv = np.asarray(uvs, np.float32)
    uv2 = uv.reshape(-1, 2)
    lam = _lambda(uv, ht, wt, mode, lod, lod_bias, mask).reshape(-1)
    idx = _indices(uv2, ht, wt, mode, np.float32)
    lev, f = _split(lam, L, np.float32)
    f = f.astype(np.float64)
    inside = (lam > 0) & (lam < L - 1)
    g = np.asarray(grad_out, np.float64).reshape(-1, ct)
    packed = np.concatenate([p.reshape(-1) for p in pyr64])
    gp, mp = np.zeros_like(packed), np.zeros_like(packed)
    n = len(uv2)
    d_u, d_v, m_u, m_v = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    sval, smag = [], []
    two = f != 0   # spec 4: where f == 0 only S_l is read and written (a NaN look-up must not put NaN * 0 into level l + 1)
    for s, (lv, wl) in enumerate(((lev, 1.0 - f), (np.minimum(lev + 1, L - 1), f))):
        look = _Look(pyr, lv, idx[:, 0], idx[:, 1], np.float32)
        fr, fc = look.fr.astype(np.float64), look.fc.astype(np.float64)
        taps = ((look.r0, look.c0, (1 - fc) * (1 - fr)), (look.r0, look.c1, fc * (1 - fr)), (look.r1, look.c0, (1 - fc) * fr), (look.r1, look.c1, fc * fr))
        sc = slice(None) if s == 0 else two
        for (r, c, w) in taps:
            fi = look.flat(r, c, ct)[sc]
            np.add.at(gp, fi, (g * (w * wl)[:, None])[sc])
            np.add.at(mp, fi, np.abs(g * (w * wl)[:, None])[sc])
        t = [packed[look.flat(r, c, ct)] for (r, c, _) in taps]   # tl, tr, bl, br
        tl, tr, bl, br = t
        d_fr = (g * ((bl - tl) * (1 - fc)[:, None] + (br - tr) * fc[:, None])).sum(-1)
        d_fc = (g * ((tr - tl) * (1 - fr)[:, None] + (br - bl) * fr[:, None])).sum(-1)
        a = np.abs
        mf_r = (a(g) * ((a(bl) + a(tl)) * (1 - fc)[:, None] + (a(br) + a(tr)) * fc[:, None])).sum(-1)
        mf_c = (a(g) * ((a(tr) + a(tl)) * (1 - fr)[:, None] + (a(br) + a(bl)) * fr[:, None])).sum(-1)
        if s == 0:
            d_v += d_fr * look.drow * wl; d_u += d_fc * look.dcol * wl
            m_v += mf_r * look.drow * a(wl); m_u += mf_c * look.dcol * a(wl)
        else:   # level l + 1 adds to (u, v) only where it carries weight, as it is scattered only there
            d_v += np.where(two, d_fr * look.drow * wl, 0.0); d_u += np.where(two, d_fc * look.dcol * wl, 0.0)
            m_v += np.where(two, mf_r * look.drow * a(wl), 0.0); m_u += np.where(two, mf_c * look.dcol * a(wl), 0.0)
        sval.append(sum(tt * ww[:, None] for tt, (_, _, ww) in zip(t, taps)))
        smag.append(sum(a(tt) * ww[:, None] for tt, (_, _, ww) in zip(t, taps)))
    u, v = uv2[:, 0], uv2[:, 1]
    if mode == 'clamp':
        du = np.where((u >= 0) & (u <= 1), wt, 0.0); dv = np.where((v >= 0) & (v <= 1), ht, 0.0)
    else:
        du = np.full(n, float(wt)); dv = np.full(n, float(ht))
    offs = np.cumsum([0] + [p.size for p in pyr])
    levels_g = [gp[offs[k]:offs[k + 1]].reshape(pyr[k].shape) for k in range(L)]
    levels_m = [mp[offs[k]:offs[k + 1]].reshape(pyr[k].shape) for k in range(L)]

    def factor(k):
        return 0.25 if (pyr[k].shape[0] > 1 and pyr[k].shape[1] > 1) else 0.5
    glod = np.where(inside, (g * (sval[1] - sval[0])).sum(-1), 0.0)
    mlod = np.where(inside, (np.abs(g) * (smag[1] + smag[0])).sum(-1), 0.0)
    return {'grad_texture': collapse(levels_g, factor), 'mass_texture': collapse(levels_m, factor),
            'grad_uvs': np.stack([d_u * du, d_v * dv], -1).reshape(uv.shape), 'mass_uvs': np.stack([m_u * du, m_v * dv], -1).reshape(uv.shape),
            'grad_lod': glod.reshape(uv.shape[:-1]), 'mass_lod': mlod.reshape(uv.shape[:-1])}
