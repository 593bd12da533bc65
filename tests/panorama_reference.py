"""A float64 numpy restatement of DESIGN.md §7k -- lat-long panoramas into cubes and back (dirt_panorama.hip,
dirt_amd/texture.py::panorama_to_cube / cube_to_panorama) -- written from the section, not from the torch form: values, both
gradients of each direction, and per output element its L1 mass (the same sums with every product's absolute value), a `kink`
flag (any of the element's samples within NEAR index units of a panorama lattice line, the u seam, an end of the clamped row, a
cube face boundary, a cube texel lattice line or an end of its clamped index, or at rho == 0) and a `jump` flag (the subset
where the VALUE itself is discontinuous: rho == 0 for a panorama look-up, a face boundary for a cube look-up, whose faces clamp
to their own edges).

`python -m tests.panorama_reference` prints the float32 torch form's worst |f32 - ref64| / mass per kind of result over CASES:
the F32 table of tests/test_panorama.py."""
import functools

import numpy as np

NEAR = 1e-3
ROTATIONS = [(0.5, 0.6, 0.2), (-0.4, 2.2, 0.3), (1.3, 0.3, 0.2)]      # angle-axis, those of tests/test_background.py
KINDS = ('out', 'd_source', 'd_rotation')

# per face: the direction of (sc, tc) is sc * FACE_S + tc * FACE_T + FACE_M; a look-up's sc = d . FACE_S, tc = d . FACE_T, a = d . FACE_M
FACE_M = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
FACE_S = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
FACE_T = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)


def rotation_matrix(w):
    """Rodrigues' formula, rounded to float32 (what the kernels are handed); None: the identity"""
    if w is None:
        return np.eye(3, dtype=np.float32)
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    k = w / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K).astype(np.float32)


def _valid(d):
    return np.isfinite(d).all(-1) & (np.abs(d).max(-1) > 0)


def _sub_centres(n, S):
    """the places (index + (a + 0.5) / S) of the n S sub-samples along an axis"""
    k = np.arange(n * S)
    return k // S + (k % S + 0.5) / S


def cube_sample_directions(N, S):
    x = 2. * _sub_centres(N, S) / N - 1.
    tc, sc = np.meshgrid(x, x, indexing='ij')
    return sc[None, ..., None] * FACE_S[:, None, None] + tc[None, ..., None] * FACE_T[:, None, None] + FACE_M[:, None, None]      # [6, N S, N S, 3]


def panorama_sample_directions(H, W, S):
    theta, phi = np.pi * _sub_centres(H, S)[:, None] / H, 2. * np.pi * (_sub_centres(W, S)[None, :] / W - 0.5)
    st = np.sin(theta)
    return np.stack([st * np.sin(phi), np.broadcast_to(np.cos(theta), (H * S, W * S)), -st * np.cos(phi)], -1)


def _blend(tex, r0, r1, c0, c1, fr, fc):
    """the four taps of every look-up [M] in tex [rows, cols, C] -> values, masses, d / d fr, d / d fc and their masses ([M, C] each), weights"""
    tl, tr, bl, br = tex[r0, c0], tex[r0, c1], tex[r1, c0], tex[r1, c1]
    fr, fc = fr[:, None], fc[:, None]
    w = [(1 - fc) * (1 - fr), fc * (1 - fr), (1 - fc) * fr, fc * fr]
    val = tl * w[0] + tr * w[1] + bl * w[2] + br * w[3]
    mass = np.abs(tl) * w[0] + np.abs(tr) * w[1] + np.abs(bl) * w[2] + np.abs(br) * w[3]
    d_fr, d_fc = (bl - tl) * (1 - fc) + (br - tr) * fc, (tr - tl) * (1 - fr) + (br - bl) * fr
    m_fr = (np.abs(bl) + np.abs(tl)) * (1 - fc) + (np.abs(br) + np.abs(tr)) * fc
    m_fc = (np.abs(tr) + np.abs(tl)) * (1 - fr) + (np.abs(br) + np.abs(bl)) * fr
    return val, mass, d_fr, m_fr, d_fc, m_fc, w


def _scatter(shape, taps, w, g):
    """g [M, C] times the four weights, added at the four taps -> (sum, its mass)"""
    out, mass = np.zeros(shape), np.zeros(shape)
    for idx, wk in zip(taps, w):
        np.add.at(out, idx, g * wk)
        np.add.at(mass, idx, np.abs(g) * wk)
    return out, mass


def look_panorama(pan, p, g=None):
    """L(p) of §7k for directions p [M, 3]; with g [M, C] (what arrives at each look-up) also the gradients"""
    Hp, Wp, C = pan.shape
    valid = _valid(p)
    x, y, z = np.where(valid[:, None], p, [0., 1., 0.]).T
    rho2 = x * x + z * z
    rho = np.sqrt(rho2)
    pole = rho == 0
    theta, phi = np.arctan2(rho, y), np.where(pole, 0., np.arctan2(x, -z))
    col, rowu = (phi / (2 * np.pi) + 0.5) * Wp - 0.5, theta / np.pi * Hp - 0.5
    inside = (rowu >= 0) & (rowu <= Hp - 1)
    row = np.clip(rowu, 0, Hp - 1)
    cf, rf = np.floor(col), np.floor(row)
    fc, fr = col - cf, row - rf
    c0 = np.mod(cf.astype(np.int64), Wp)
    c1, r0 = np.mod(c0 + 1, Wp), rf.astype(np.int64)
    r1 = np.minimum(r0 + 1, Hp - 1)
    val, mass, d_fr, m_fr, d_fc, m_fc, w = _blend(pan, r0, r1, c0, c1, fr, fc)
    near_row = np.where(inside, np.minimum(fr, 1 - fr), np.minimum(np.abs(rowu), np.abs(rowu - (Hp - 1))))
    near = np.minimum(np.minimum(fc, 1 - fc), np.minimum(col + 0.5, Wp - 0.5 - col))
    res = {'value': val * valid[:, None], 'mass': mass * valid[:, None], 'kink': valid & ((np.minimum(near, near_row) < NEAR) | pole), 'jump': valid & pole,
           'valid': valid, 'box': (r0, r1, np.minimum(c0, c1), np.maximum(c0, c1))}
    if g is None:
        return res
    g = g * valid[:, None]
    taps = [(r0, c0), (r0, c1), (r1, c0), (r1, c1)]
    res['d_source'], res['mass_d_source'] = _scatter(pan.shape, taps, w, g)
    live = ~pole
    safe2, safe = np.where(live, rho2, 1.), np.where(live, rho, 1.)
    n2 = safe2 + y * y
    out, mass = np.zeros_like(p), np.zeros_like(p)
    for grad, m, scale, vec in (((g * d_fc).sum(-1), (np.abs(g) * m_fc).sum(-1), Wp / (2 * np.pi), np.stack([-z, 0 * z, x], -1) / safe2[:, None]),
                                ((g * d_fr).sum(-1) * inside, (np.abs(g) * m_fr).sum(-1) * inside, Hp / np.pi,
                                 np.stack([x * y / safe, -safe, z * y / safe], -1) / n2[:, None])):
        out += (grad * scale * live)[:, None] * vec
        mass += (m * scale * live)[:, None] * np.abs(vec)
    res['d_direction'], res['mass_d_direction'] = out, mass
    return res


def look_cube(cube, q, g=None):
    """the bilinear cube look-up (spec 2 - 4 and 6 of dirt_texture_cube.hip) of directions q [M, 3]"""
    N, C = cube.shape[1], cube.shape[3]
    valid = _valid(q)
    d = np.where(valid[:, None], q, [1., 0., 0.])
    ad = np.abs(d)
    major = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    face = 2 * major + (d[np.arange(len(d)), major] <= 0)
    a = (d * FACE_M[face]).sum(-1)
    s, t = (d * FACE_S[face]).sum(-1) / a, (d * FACE_T[face]).sum(-1) / a
    second = np.sort(ad, -1)[:, 1] / a
    idx, slope, near = [], [], (1 - second) * N / 2
    for coordinate in (t, s):      # row, column
        raw = ((coordinate + 1) * 0.5) * N - 0.5
        into = (raw >= 0) & (raw <= N - 1)
        c = np.clip(raw, 0, N - 1)
        frac = c - np.floor(c)
        near = np.minimum(near, np.where(into, np.minimum(frac, 1 - frac), np.minimum(np.abs(raw), np.abs(raw - (N - 1)))))
        idx.append(c)
        slope.append(np.where(into, N / 2., 0.))
    rf, cf = np.floor(idx[0]), np.floor(idx[1])
    fr, fc = idx[0] - rf, idx[1] - cf
    r0, c0 = rf.astype(np.int64), cf.astype(np.int64)
    r1, c1 = np.minimum(r0 + 1, N - 1), np.minimum(c0 + 1, N - 1)
    flat = cube.reshape(6 * N, N, C)
    val, mass, d_fr, m_fr, d_fc, m_fc, w = _blend(flat, face * N + r0, face * N + r1, c0, c1, fr, fc)
    res = {'value': val * valid[:, None], 'mass': mass * valid[:, None], 'kink': valid & (near < NEAR), 'jump': valid & ((1 - second) * N / 2 < NEAR),
           'valid': valid}
    if g is None:
        return res
    g = g * valid[:, None]
    taps = [(face * N + r0, c0), (face * N + r0, c1), (face * N + r1, c0), (face * N + r1, c1)]
    ds, ms = _scatter(flat.shape, taps, w, g)
    res['d_source'], res['mass_d_source'] = ds.reshape(cube.shape), ms.reshape(cube.shape)
    gs, gt = (g * d_fc).sum(-1) * slope[1], (g * d_fr).sum(-1) * slope[0]
    ms_, mt_ = (np.abs(g) * m_fc).sum(-1) * slope[1], (np.abs(g) * m_fr).sum(-1) * slope[0]
    g_a, m_a = -(gs * s + gt * t) / a, (ms_ * np.abs(s) + mt_ * np.abs(t)) / a
    res['d_direction'] = (gs / a)[:, None] * FACE_S[face] + (gt / a)[:, None] * FACE_T[face] + g_a[:, None] * FACE_M[face]
    res['mass_d_direction'] = (ms_ / a)[:, None] * np.abs(FACE_S[face]) + (mt_ / a)[:, None] * np.abs(FACE_T[face]) + m_a[:, None] * np.abs(FACE_M[face])
    return res


def _resample(look, source, directions, rotation, to_cube, S, grad_out):
    """directions [..., R S, C S, 3] of the samples -> the keys of a result; `rotation` float32 values, taken as they are"""
    R = np.asarray(rotation, np.float64)
    lead = directions.shape[:-3]
    rows, cols = directions.shape[-3] // S, directions.shape[-2] // S
    flat = directions.reshape(-1, 3)
    turned = flat @ (R.T if to_cube else R)
    C = source.shape[-1]
    g = None
    if grad_out is not None:
        g = np.repeat(np.repeat(np.asarray(grad_out, np.float64), S, -3), S, -2).reshape(-1, C) / (S * S)
    got = look(source.astype(np.float64), turned, g)

    def mean(x, ch):
        return x.reshape(lead + (rows, S, cols, S) + ((ch,) if ch else ())).sum((-4, -2) if ch else (-3, -1))

    res = {'out': mean(got['value'], C) / (S * S), 'mass_out': mean(got['mass'], C) / (S * S), 'kink': mean(got['kink'], 0) > 0,
           'jump': mean(got['jump'], 0) > 0, 'valid': got['valid'].reshape(lead + (rows * S, cols * S))}
    if g is not None:
        res['d_source'], res['mass_d_source'] = got['d_source'], got['mass_d_source']
        gd, md = got['d_direction'], got['mass_d_direction']
        if to_cube:      # p_k = sum_j e_j R[k][j]
            res['d_rotation'], res['mass_d_rotation'] = gd.T @ flat, md.T @ np.abs(flat)
        else:            # q_k = sum_j d_j R[j][k]
            res['d_rotation'], res['mass_d_rotation'] = flat.T @ gd, np.abs(flat).T @ md
    return res


def panorama_to_cube(panorama, size, samples=1, rotation=None, grad_out=None):
    rotation = np.eye(3) if rotation is None else rotation
    return _resample(look_panorama, panorama, cube_sample_directions(size, samples), rotation, True, samples, grad_out)


def cube_to_panorama(cube, height, width, samples=1, rotation=None, grad_out=None):
    rotation = np.eye(3) if rotation is None else rotation
    return _resample(look_cube, cube, panorama_sample_directions(height, width, samples), rotation, False, samples, grad_out)


# ---- the cases: (direction, source shape, output sizes, samples, rotation index or None, seed)

class Case:
    """One call: the source (float32 values), the sizes, the rotation (float32 [3, 3]; `turned`: whether d rotation is compared
    and the kinks excluded -- the identity puts whole sample rows on lattice lines, so it is tested for values and d source
    alone), and an incoming gradient that is zero on the excluded elements"""

    def __init__(self, to_cube, source_shape, sizes, samples, rotation, seed):
        rng = np.random.default_rng(seed)
        self.to_cube, self.sizes, self.samples, self.turned = to_cube, sizes, samples, rotation is not None
        self.source = rng.standard_normal(source_shape).astype(np.float32)
        self.rotation = rotation_matrix(None if rotation is None else ROTATIONS[rotation])
        plain = self.run(None)
        self.excluded = plain['kink'] if self.turned else plain['jump']
        self.share = float(self.excluded.mean())
        go = rng.standard_normal(plain['out'].shape).astype(np.float32)
        go[self.excluded] = 0.
        self.go = go

    def run(self, grad_out):
        if self.to_cube:
            return panorama_to_cube(self.source, self.sizes, self.samples, self.rotation, grad_out)
        return cube_to_panorama(self.source, self.sizes[0], self.sizes[1], self.samples, self.rotation, grad_out)

    @functools.cached_property
    def ref(self):
        return self.run(self.go)

    @property
    def kinds(self):
        return KINDS if self.turned else KINDS[:2]


def _to_cube(pano, n, s, c, rotation, seed):
    return lambda: Case(True, pano + (c,), n, s, rotation, seed)


def _to_pano(n, size, s, c, rotation, seed):
    return lambda: Case(False, (6, n, n, c), size, s, rotation, seed)


_CASES = {
    # the rows of the issue's table of excluded shares, each under the three rotations
    **{'n4-s4-r%d' % k: _to_cube((6, 11), 4, 4, 3, k, 10 + k) for k in range(3)},
    **{'n5-s3-r%d' % k: _to_cube((7, 13), 5, 3, 3, k, 20 + k) for k in range(3)},
    **{'n8-s2-r%d' % k: _to_cube((16, 32), 8, 2, 4, k, 30 + k) for k in range(3)},
    **{'n17-s2-r%d' % k: _to_cube((9, 20), 17, 2, 1, k, 40 + k) for k in range(3)},      # a 16 x 16 tile and one past it; the seam and a pole cross tiles
    **{'n16-s1-r%d' % k: _to_cube((64, 128), 16, 1, 3, k, 50 + k) for k in range(3)},
    'n1-s4': _to_cube((6, 11), 1, 4, 3, 0, 60),
    'minify': _to_cube((64, 128), 4, 2, 3, 2, 61),                  # a tile's taps span more than the LDS patch
    'c5': _to_cube((7, 13), 5, 2, 5, 0, 62),                        # any channel count: one channel per pass
    'p1x1': _to_cube((1, 1), 5, 1, 3, 1, 63),
    'p1x7': _to_cube((1, 7), 5, 2, 3, 2, 64),                       # every row clamps
    'p5x1': _to_cube((5, 1), 5, 2, 3, 0, 65),                       # both column taps are one texel
    'p5x2': _to_cube((5, 2), 5, 3, 4, 1, 66),                       # ... or each other's wrap
    'id-n5-s3': _to_cube((7, 13), 5, 3, 3, None, 67),               # N S odd: the centre sample of +-Y is the pole itself
    'id-n16-s1': _to_cube((16, 32), 16, 1, 3, None, 68),
    'id-n17-s2': _to_cube((9, 20), 17, 2, 4, None, 69),
    'q1x1': _to_pano(4, (1, 1), 3, 3, 0, 80),
    'q3x5': _to_pano(1, (3, 5), 2, 1, 1, 81),
    'q16x16': _to_pano(9, (16, 16), 1, 3, 2, 82),
    'q17x33': _to_pano(4, (17, 33), 2, 4, 0, 83),
    'q1x300': _to_pano(9, (1, 300), 2, 3, 1, 84),                   # a one-row panorama: tiles of 256 x 1, and one past the first
    'q-c5': _to_pano(9, (3, 5), 4, 5, 1, 85),
    'q-s3': _to_pano(4, (16, 16), 3, 3, 2, 86),
    'q-id': _to_pano(9, (17, 33), 1, 3, None, 87),
}
CASES = list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


# ---- comparing a result with the restatement

def worst_ratio(got, ref, mass, keep=None):
    """the largest |got - ref| / mass over the elements of positive mass that `keep` keeps"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    on = mass > 0
    if keep is not None:
        on = on & keep
    return float((err[on] / mass[on]).max()) if on.any() else 0.


def ratios(got, c):
    """per kind of result in `got`: its worst ratio.  The excluded elements of `out` are not compared"""
    ref = c.ref
    keep = np.broadcast_to(~c.excluded[..., None], ref['out'].shape)
    out = {'out': worst_ratio(got['out'], ref['out'], ref['mass_out'], keep)}
    for kind in c.kinds[1:]:
        if got.get(kind) is not None:
            out[kind] = worst_ratio(got[kind], ref[kind], ref['mass_' + kind])
    return out


def exact_where_massless(got, c):
    ref = c.ref
    keep = np.broadcast_to(~c.excluded[..., None], ref['out'].shape)
    ok = not np.asarray(got['out'])[keep & (ref['mass_out'] == 0)].any()
    for kind in c.kinds[1:]:
        if got.get(kind) is not None:
            ok = ok and not np.asarray(got[kind])[ref['mass_' + kind] == 0].any()
    return ok


def torch_form(c, dtype=None):
    """the case through dirt_amd.texture's dense forms on the CPU, gradients by autograd -> the keys of KINDS"""
    import torch
    from dirt_amd import texture
    dtype = dtype or torch.float32
    source, rotation = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (c.source, c.rotation))
    if c.to_cube:
        out = texture.panorama_to_cube_dense(source, c.sizes, c.samples, rotation)
    else:
        out = texture.cube_to_panorama_dense(source, c.sizes[0], c.sizes[1], c.samples, rotation)
    out.backward(torch.tensor(c.go, dtype=dtype))
    return {'out': out.detach().numpy(), 'd_source': source.grad.numpy(), 'd_rotation': rotation.grad.numpy()}


if __name__ == '__main__':
    table = {}
    for name in CASES:
        c = case(name)
        worst = ratios(torch_form(c), c)
        print('%-12s share %.3f  %s' % (name, c.share, {k: '%.2e' % v for k, v in worst.items()}))
        for k, v in worst.items():
            key = ('cube_' if c.to_cube else 'panorama_') + k
            table[key] = max(table.get(key, 0.), v)
    print('F32 =', {k: float('%.2e' % (v * 1.005)) for k, v in sorted(table.items())})      # (rounded up: the table bounds its own cases)
