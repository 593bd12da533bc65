"""numpy restatement of the cube-map look-up -- TEST INFRASTRUCTURE: dirt_amd never imports it.

The specification is DESIGN.md §7 (and the header of dirt_amd/csrc/dirt_texture_cube.hip): the face of a direction by its major
axis, the GL texel-centre index ((sc / a + 1) * 0.5) * n - 0.5 clamped to the face, the bilinear blend of tests/mip_reference.py
(whose pyramid, level split and collapse are used as they are, per face), 0 for a direction that is not finite or all zero.
`Look`, `index` and the taps follow the kernels' float32 operations one by one, so face, floor and 'nearest' agree with them bit for
bit (dtype=np.float64 gives the same expressions in double precision, for finite differences); `grad` is the analytic gradient,
accumulated in float64, with the L1 mass of each element's terms."""
import numpy as np

from tests import mip_reference as mr


class Look:
    """Per direction (flattened to [n]): valid, face (0 where not valid), major axis, pos (major component > 0), a = |major
    component|, s = sc / a and t = tc / a (0 where not valid)."""

    def __init__(self, directions, dt=np.float32):
        d = np.asarray(directions, dt).reshape(-1, 3)
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
            is_x = (ax >= ay) & (ax >= az)
            is_y = ~is_x & (ay >= az)
            a = np.where(is_x, ax, np.where(is_y, ay, az))
            pos = np.where(is_x, x, np.where(is_y, y, z)) > 0
            self.valid = np.isfinite(d).all(-1) & (a > 0)
            sc = np.where(is_x, np.where(pos, -z, z), np.where(is_y, x, np.where(pos, x, -x)))
            tc = np.where(is_y, np.where(pos, z, -z), -y)
            self.a = np.where(self.valid, a, dt(1)).astype(dt)
            self.s = np.where(self.valid, sc / self.a, dt(0)).astype(dt)
            self.t = np.where(self.valid, tc / self.a, dt(0)).astype(dt)
        self.major = np.where(is_x, 0, np.where(is_y, 1, 2))
        self.pos = pos
        self.face = np.where(self.valid, 2 * self.major + (~pos), 0).astype(np.int64)


def index(s, n, dt=np.float32):
    """s = sc / a (or tc / a) -> (index at a level of size n, clamped to [0, n - 1]; d index / d s: n / 2 where the unclamped value
    lies in [0, n - 1], else 0).  n: an int or an array per look-up."""
    nf = np.asarray(n).astype(dt)
    x = ((((s + dt(1)) * dt(0.5)).astype(dt) * nf).astype(dt) - dt(0.5)).astype(dt)
    top = (nf - dt(1)).astype(dt)
    d = np.where((x >= 0) & (x <= top), 0.5 * np.asarray(n, np.float64), 0.0)
    return np.where(x < 0, dt(0), np.where(x > top, top, x)).astype(dt), d


def cube_indices(directions, size, dt=np.float32):
    """-> (face [...], (row, col) [..., 2], valid [...]): what dirt_amd.texture.directions_to_cube_indices returns."""
    q = Look(directions, dt)
    row, col = index(q.t, size, dt)[0], index(q.s, size, dt)[0]
    shape = np.asarray(directions).shape[:-1]
    idx = np.where(q.valid[:, None], np.stack([row, col], -1), dt(0)).astype(dt)
    return q.face.reshape(shape), idx.reshape(shape + (2,)), q.valid.reshape(shape)


class _Set:
    """One tap set per look-up: the level `lev` [n] of each look-up's face, its taps, fractions and index derivatives."""

    def __init__(self, q, dims, offs, floats, lev, nearest, dt):
        self.n = np.asarray(dims)[lev]
        row, self.drow = index(q.t, self.n, dt)
        col, self.dcol = index(q.s, self.n, dt)
        self.r0, self.r1, self.c0, self.c1, self.fr, self.fc = mr._taps(row, col, self.n, self.n, dt)
        if nearest:   # texel_index(index + 0.5): one tap of weight 1
            self.r0 = self.r1 = np.minimum(np.floor((row + dt(0.5)).astype(dt)).astype(np.int64), self.n - 1)
            self.c0 = self.c1 = np.minimum(np.floor((col + dt(0.5)).astype(dt)).astype(np.int64), self.n - 1)
            self.fr, self.fc = np.zeros_like(row), np.zeros_like(col)
        self.base = q.face * floats + np.asarray(offs)[lev]

    def flat(self, r, c, ct):   # flat indices into the packed pyramids [6 * floats] -> [n, ct]
        return (self.base + (r * self.n + c) * ct)[:, None] + np.arange(ct)[None, :]

    def taps(self, dt=np.float64):
        fr, fc = self.fr.astype(dt), self.fc.astype(dt)
        return ((self.r0, self.c0, (1 - fc) * (1 - fr)), (self.r0, self.c1, fc * (1 - fr)), (self.r1, self.c0, (1 - fc) * fr), (self.r1, self.c1, fc * fr))


def _setup(cube, directions, filter, lod, lod_bias, max_level, dt):
    """-> (look, packed pyramids [6 * floats] in dt, level sizes, level offsets, floats per face, level [n], fraction [n], lambda [n])"""
    cube = np.asarray(cube, dt)
    assert cube.ndim == 4 and cube.shape[0] == 6 and cube.shape[1] == cube.shape[2]
    assert filter in ('bilinear', 'nearest', 'trilinear') and (filter == 'trilinear') == (lod is not None)
    pyrs = [mr.pyramid(cube[f], max_level if filter == 'trilinear' else 0, dt) for f in range(6)]
    dims = [p.shape[0] for p in pyrs[0]]
    sizes = [p.size for p in pyrs[0]]
    offs, floats = np.cumsum([0] + sizes)[:-1], int(sum(sizes))
    packed = np.concatenate([p.reshape(-1) for pyr in pyrs for p in pyr])
    q = Look(directions, dt)
    n = len(q.valid)
    if lod is None:
        return q, packed, dims, offs, floats, np.zeros(n, np.int64), np.zeros(n, dt), np.zeros(n, dt)
    with np.errstate(invalid='ignore'):
        lam = (np.asarray(lod, dt).reshape(-1) + dt(lod_bias)).astype(dt)
        lev, f = mr._split(lam, len(dims), dt)
    return q, packed, dims, offs, floats, lev, f, lam


def sample(cube, directions, filter='bilinear', lod=None, lod_bias=0.0, max_level=None, dtype=np.float32, magnitude=False):
    """The look-up [..., C]; magnitude=True also returns the same blend of |pyramid| in float64 (the value's scale)."""
    dt = dtype
    q, packed, dims, offs, floats, lev, f, _ = _setup(cube, directions, filter, lod, lod_bias, max_level, dt)
    ct = np.asarray(cube).shape[3]
    one = dt(1)

    def bil(st, src):
        a, b = src[st.flat(st.r0, st.c0, ct)], src[st.flat(st.r0, st.c1, ct)]
        c, d = src[st.flat(st.r1, st.c0, ct)], src[st.flat(st.r1, st.c1, ct)]
        if filter == 'nearest':
            return a
        fr, fc = st.fr[:, None], st.fc[:, None]
        wr0, wc0 = one - fr, one - fc
        return ((((a * wc0) * wr0) + ((b * fc) * wr0)) + ((c * wc0) * fr)) + ((d * fc) * fr)

    s0 = _Set(q, dims, offs, floats, lev, filter == 'nearest', dt)
    s1 = _Set(q, dims, offs, floats, np.minimum(lev + 1, len(dims) - 1), False, dt)
    v0, v1, fv = bil(s0, packed), bil(s1, packed), f[:, None]
    with np.errstate(invalid='ignore'):
        out = np.where(fv == 0, v0, (one - fv) * v0 + fv * v1).astype(dt)
    out = np.where(q.valid[:, None], out, dt(0)).astype(dt)
    shape = np.asarray(directions).shape[:-1] + (ct,)
    if not magnitude:
        return out.reshape(shape)
    m0, m1, f64 = bil(s0, np.abs(packed)).astype(np.float64), bil(s1, np.abs(packed)).astype(np.float64), fv.astype(np.float64)
    mag = np.where(f64 == 0, m0, (1 - f64) * m0 + f64 * m1)
    return out.reshape(shape), np.where(q.valid[:, None], mag, 0.0).reshape(shape)


def level0_taps(directions, size):
    """-> (valid, face, r0, r1, c0, c1) per direction [n]: the texels a bilinear look-up touches (the backward's tile classes)."""
    q = Look(directions)
    st = _Set(q, [size], [0], size * size, np.zeros(len(q.valid), np.int64), False, np.float32)
    return q.valid, q.face, st.r0, st.r1, st.c0, st.c1


def direction_gradient(q, gs, gt):
    """dL/d(sc / a), dL/d(tc / a) [n] -> dL/d(x, y, z) [n, 3] in float64, for the looks `q`: sc and tc over a, and a = |major component|."""
    a, s, t = q.a.astype(np.float64), q.s.astype(np.float64), q.t.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        g_sc, g_tc = gs / a, gt / a
        g_m = np.where(q.pos, -1.0, 1.0) * ((gs * s + gt * t) / a)
    mx, my, sg = q.major == 0, q.major == 1, np.where(q.pos, 1.0, -1.0)
    gx = np.where(mx, g_m, np.where(my, g_sc, sg * g_sc))
    gy = np.where(my, g_m, -g_tc)
    gz = np.where(mx, -sg * g_sc, np.where(my, sg * g_tc, g_m))
    return np.stack([gx, gy, gz], -1)


def grad(cube, directions, grad_out, filter='bilinear', lod=None, lod_bias=0.0, max_level=None):
    """-> dict grad_cube, grad_directions, grad_lod (float64) and mass_cube, mass_directions, mass_lod (their terms' L1 mass)."""
    q, packed32, dims, offs, floats, lev, f, lam = _setup(cube, directions, filter, lod, lod_bias, max_level, np.float32)
    packed = packed32.astype(np.float64)
    L, ct = len(dims), np.asarray(cube).shape[3]
    n = len(q.valid)
    f = f.astype(np.float64)
    with np.errstate(invalid='ignore'):
        inside = (lam > 0) & (lam < L - 1) & q.valid
    g = np.where(q.valid[:, None], np.asarray(grad_out, np.float64).reshape(-1, ct), 0.0)   # an invalid look-up adds to nothing
    gp, mp = np.zeros_like(packed), np.zeros_like(packed)
    gs, gt, ms, mt = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    sval, smag = [], []
    two = (f != 0) & q.valid
    a = np.abs
    for s, (lv, wl) in enumerate(((lev, 1.0 - f), (np.minimum(lev + 1, L - 1), f))):
        st = _Set(q, dims, offs, floats, lv, filter == 'nearest', np.float32)
        fr, fc = st.fr.astype(np.float64), st.fc.astype(np.float64)
        taps = st.taps()
        on = q.valid if s == 0 else two
        for (r, c, w) in taps:
            fi = st.flat(r, c, ct)[on]
            np.add.at(gp, fi, (g * (w * wl)[:, None])[on])
            np.add.at(mp, fi, a(g * (w * wl)[:, None])[on])
        tl, tr, bl, br = t4 = [packed[st.flat(r, c, ct)] for (r, c, _) in taps]
        d_fr = (g * ((bl - tl) * (1 - fc)[:, None] + (br - tr) * fc[:, None])).sum(-1)
        d_fc = (g * ((tr - tl) * (1 - fr)[:, None] + (br - bl) * fr[:, None])).sum(-1)
        mf_r = (a(g) * ((a(bl) + a(tl)) * (1 - fc)[:, None] + (a(br) + a(tr)) * fc[:, None])).sum(-1)
        mf_c = (a(g) * ((a(tr) + a(tl)) * (1 - fr)[:, None] + (a(br) + a(bl)) * fr[:, None])).sum(-1)
        if filter != 'nearest':   # floor() has zero gradient; the nearest texel none at all
            gt += np.where(on, d_fr * st.drow * wl, 0.0); gs += np.where(on, d_fc * st.dcol * wl, 0.0)
            mt += np.where(on, mf_r * st.drow * a(wl), 0.0); ms += np.where(on, mf_c * st.dcol * a(wl), 0.0)
        sval.append(sum(tt * ww[:, None] for tt, (_, _, ww) in zip(t4, taps)))
        smag.append(sum(a(tt) * ww[:, None] for tt, (_, _, ww) in zip(t4, taps)))
    gd = np.where(q.valid[:, None], direction_gradient(q, gs, gt), 0.0)
    a64, s64, t64 = q.a.astype(np.float64), a(q.s.astype(np.float64)), a(q.t.astype(np.float64))
    with np.errstate(over='ignore', invalid='ignore'):
        m_sc, m_tc, m_m = ms / a64, mt / a64, (ms * s64 + mt * t64) / a64
    mx, my = q.major == 0, q.major == 1
    md = np.stack([np.where(mx, m_m, m_sc), np.where(my, m_m, m_tc), np.where(mx, m_sc, np.where(my, m_tc, m_m))], -1)
    md = np.where(q.valid[:, None], md, 0.0)

    def to_cube(x):   # every level's gradient of every face -> the cube's
        faces = []
        for fc_ in range(6):
            levels = [x[fc_ * floats + offs[k]:fc_ * floats + offs[k] + dims[k] * dims[k] * ct].reshape(dims[k], dims[k], ct) for k in range(L)]
            faces.append(mr.collapse(levels, lambda k: 0.25))
        return np.stack(faces)

    shape = np.asarray(directions).shape
    glod = np.where(inside, (g * (sval[1] - sval[0])).sum(-1), 0.0)
    mlod = np.where(inside, (a(g) * (smag[1] + smag[0])).sum(-1), 0.0)
    return {'grad_cube': to_cube(gp), 'mass_cube': to_cube(mp), 'grad_directions': gd.reshape(shape), 'mass_directions': md.reshape(shape),
            'grad_lod': glod.reshape(shape[:-1]), 'mass_lod': mlod.reshape(shape[:-1])}
