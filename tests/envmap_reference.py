"""numpy float64 restatement of the environment prefilter -- TEST INFRASTRUCTURE: dirt_amd never imports it.

The specification is DESIGN.md §7 "Environment prefilter" (and the header of dirt_amd/csrc/dirt_envmap.hip):

  texel direction   face f, row r, column c of an n x n face: sc = 2 (c + 0.5) / n - 1, tc = 2 (r + 0.5) / n - 1, the vector
                    +X (1, -tc, -sc), -X (-1, -tc, sc), +Y (sc, 1, tc), -Y (sc, -1, -tc), +Z (sc, -tc, 1), -Z (-sc, -tc, -1)
                    normalised; solid-angle weight W = (1 + sc^2 + tc^2)^(-3/2);
  kernel weight     t = d_o . d_s, t+ = max(t, 0); 'lambert': k = t+; 'ggx', alpha = roughness^2: q(t) = 1 / (1 + t+^2 (alpha^2 - 1))^2,
                    q_c = q(t_c) with t_c^2 = (1 - 16 alpha^2) / (1 - alpha^2) if 16 alpha^2 < 1, else 0; k = t+ max(q(t) - q_c, 0);
  convolution       Z_o = sum_s k(t_os) W_s, out[o, c] = sum_s k(t_os) W_s S[s, c] / Z_o; roughness 0: the identity;
  transpose         grad_S[s, c] = W_s sum_o k(t_os) grad_out[o, c] / Z_o;
  pyramid           the box pyramid per face (tests/mip_reference.py), level k convolved at roughness[k], default k / (L - 1).

`weight_matrix` is the normalised matrix k W / Z of one level [6 n^2, 6 n^2], cached for the few cases in use at a time; the
look-up of a pyramid is tests/cube_reference.py's arithmetic on levels given by the caller."""
import functools

import numpy as np

from tests import cube_reference as cr
from tests import mip_reference as mr

TILE = 16   # the kernel's tile: live_tile_pairs counts what its cull has to keep


def texel_directions(n):
    """-> (directions [6, n, n, 3], weights [6, n, n]) in float64."""
    x = 2.0 * (np.arange(n, dtype=np.float64) + 0.5) / n - 1.0
    tc, sc = np.meshgrid(x, x, indexing='ij')
    one = np.ones_like(sc)
    v = np.stack([np.stack(f, -1) for f in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one))])
    norm2 = 1.0 + sc * sc + tc * tc
    return v / np.sqrt(norm2)[None, :, :, None], np.broadcast_to(norm2 ** -1.5, (6, n, n)).copy()


def cutoff(roughness):
    """-> (alpha^2, q_c, t_c) of a GGX lobe."""
    a2 = float(roughness) ** 4
    if 16.0 * a2 < 1.0:
        tc2 = (1.0 - 16.0 * a2) / (1.0 - a2)
        return a2, 1.0 / (1.0 + tc2 * (a2 - 1.0)) ** 2, np.sqrt(tc2)
    return a2, 0.0, 0.0


@functools.lru_cache(maxsize=3)
def weight_matrix(n, roughness, kind):
    """The normalised weights [6 n^2 outputs, 6 n^2 sources] of one level: k(t_os) W_s / Z_o.  roughness 0: the identity."""
    assert kind in ('ggx', 'lambert')
    m = 6 * n * n
    if kind == 'ggx' and roughness == 0:
        return np.eye(m)
    d, w = texel_directions(n)
    d = d.reshape(m, 3)
    t = d @ d.T
    np.maximum(t, 0.0, out=t)
    if kind == 'ggx':
        a2, qc, _ = cutoff(roughness)
        q = t * t
        q *= a2 - 1.0
        q += 1.0
        np.square(q, out=q)
        np.reciprocal(q, out=q)
        q -= qc
        np.maximum(q, 0.0, out=q)
        t *= q
        del q
    t *= w.reshape(1, m)
    z = t.sum(1, keepdims=True)
    assert (z > 0).all()
    t /= z
    t.setflags(write=False)
    return t


def live_tile_pairs(n, roughness, kind):
    """-> (pairs of TILE x TILE tiles with a pair of texels of non-zero weight, all pairs)."""
    tiles = -(-n // TILE)
    tile = (np.arange(n) // TILE)
    ids = (np.arange(6)[:, None, None] * tiles + tile[None, :, None]) * tiles + tile[None, None, :]
    ids = ids.reshape(-1)
    count = 6 * tiles * tiles
    hit = np.zeros((count, count), bool)
    o, s = np.nonzero(weight_matrix(n, roughness, kind) > 0)
    hit[ids[o], ids[s]] = True
    return int(hit.sum()), count * count


def convolve(cube, roughness=None, kind='ggx'):
    """cube [6, n, n, C] -> (out [6, n, n, C] in float64, the L1 mass of each element's terms)."""
    cube = np.asarray(cube, np.float64)
    w = weight_matrix(cube.shape[1], None if kind == 'lambert' else float(roughness), kind)
    flat = cube.reshape(-1, cube.shape[3])
    return (w @ flat).reshape(cube.shape), (w @ np.abs(flat)).reshape(cube.shape)


def convolve_grad(grad_out, roughness=None, kind='ggx'):
    """grad_out [6, n, n, C] -> (grad_cube, its elements' L1 mass): the transpose."""
    g = np.asarray(grad_out, np.float64)
    w = weight_matrix(g.shape[1], None if kind == 'lambert' else float(roughness), kind)
    flat = g.reshape(-1, g.shape[3])
    return (w.T @ flat).reshape(g.shape), (w.T @ np.abs(flat)).reshape(g.shape)


def default_roughness(levels):
    return tuple(k / (levels - 1) for k in range(levels)) if levels > 1 else (0.0,)


def box_levels(cube, max_level=None):
    """The box pyramid of the six faces in float32 (the bits the build kernel gives) -> [level k: [6, n_k, n_k, C]]."""
    pyrs = [mr.pyramid(np.asarray(cube, np.float32)[f], max_level, np.float32) for f in range(6)]
    return [np.stack([pyrs[f][k] for f in range(6)]) for k in range(len(pyrs[0]))]


def prefilter(cube, roughness=None, max_level=None):
    """-> [level k [6, n_k, n_k, C] float64]: the box pyramid, level k convolved at roughness[k]."""
    box = box_levels(cube, max_level)
    roughness = default_roughness(len(box)) if roughness is None else roughness
    assert len(roughness) == len(box)
    return [convolve(lv, r)[0] for lv, r in zip(box, roughness)]


def prefilter_grad(grad_levels, mass_levels, roughness):
    """The gradient (and its mass) of every level of the prefiltered pyramid -> the cube's: the transposed convolution per level,
    then the box pyramid's collapse per face."""
    g = [weight_matrix(x.shape[1], float(r), 'ggx').T @ x.reshape(-1, x.shape[3]) for x, r in zip(grad_levels, roughness)]
    m = [weight_matrix(x.shape[1], float(r), 'ggx').T @ x.reshape(-1, x.shape[3]) for x, r in zip(mass_levels, roughness)]
    g = [a.reshape(x.shape) for a, x in zip(g, grad_levels)]
    m = [a.reshape(x.shape) for a, x in zip(m, grad_levels)]
    collapse = lambda lv: np.stack([mr.collapse([x[f] for x in lv], lambda k: 0.25) for f in range(6)])   # noqa: E731
    return collapse(g), collapse(m)


def lookup_grad(levels, directions, lod, grad_out):
    """The trilinear cube look-up in the pyramid `levels` (float64; tests/cube_reference.py's `grad` with the levels given, its
    indices and level split in float32 as the kernels take them) -> dict: out, and grad_levels, grad_directions, grad_lod with
    mass_levels, mass_directions, mass_lod."""
    levels = [np.asarray(x, np.float64) for x in levels]
    L, ct = len(levels), levels[0].shape[3]
    dims = [x.shape[1] for x in levels]
    sizes = [x[0].size for x in levels]
    offs, floats = np.cumsum([0] + sizes)[:-1], int(sum(sizes))
    packed = np.concatenate([x[f].reshape(-1) for f in range(6) for x in levels])
    q = cr.Look(directions, np.float32)
    n = len(q.valid)
    lam = np.asarray(lod, np.float32).reshape(-1)
    with np.errstate(invalid='ignore'):
        lev, f = mr._split(lam, L, np.float32)
        inside = (lam > 0) & (lam < L - 1) & q.valid
    f = f.astype(np.float64)
    g = np.where(q.valid[:, None], np.asarray(grad_out, np.float64).reshape(-1, ct), 0.0)
    gp, mp = np.zeros_like(packed), np.zeros_like(packed)
    gs, gt, ms, mt = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    sval, smag = [], []
    two = (f != 0) & q.valid
    a = np.abs
    for s, (lv, wl) in enumerate(((lev, 1.0 - f), (np.minimum(lev + 1, L - 1), f))):
        st = cr._Set(q, dims, offs, floats, lv, False, np.float32)
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
        gt += np.where(on, d_fr * st.drow * wl, 0.0); gs += np.where(on, d_fc * st.dcol * wl, 0.0)
        mt += np.where(on, mf_r * st.drow * a(wl), 0.0); ms += np.where(on, mf_c * st.dcol * a(wl), 0.0)
        sval.append(sum(tt * ww[:, None] for tt, (_, _, ww) in zip(t4, taps)))
        smag.append(sum(a(tt) * ww[:, None] for tt, (_, _, ww) in zip(t4, taps)))
    gd = np.where(q.valid[:, None], cr.direction_gradient(q, gs, gt), 0.0)
    a64, s64, t64 = q.a.astype(np.float64), a(q.s.astype(np.float64)), a(q.t.astype(np.float64))
    with np.errstate(over='ignore', invalid='ignore'):
        m_sc, m_tc, m_m = ms / a64, mt / a64, (ms * s64 + mt * t64) / a64
    mx, my = q.major == 0, q.major == 1
    md = np.stack([np.where(mx, m_m, m_sc), np.where(my, m_m, m_tc), np.where(mx, m_sc, np.where(my, m_tc, m_m))], -1)
    md = np.where(q.valid[:, None], md, 0.0)

    def unpack(x):
        x = x.reshape(6, floats)
        return [x[:, offs[k]:offs[k] + sizes[k]].reshape(6, dims[k], dims[k], ct) for k in range(L)]

    fv = f[:, None]
    out = np.where(q.valid[:, None], (1 - fv) * sval[0] + fv * sval[1], 0.0)
    mag = np.where(q.valid[:, None], (1 - fv) * smag[0] + fv * smag[1], 0.0)
    shape = np.asarray(directions).shape
    return {'out': out.reshape(shape[:-1] + (ct,)), 'mag': mag.reshape(shape[:-1] + (ct,)),
            'grad_levels': unpack(gp), 'mass_levels': unpack(mp), 'grad_directions': gd.reshape(shape), 'mass_directions': md.reshape(shape),
            'grad_lod': np.where(inside, (g * (sval[1] - sval[0])).sum(-1), 0.0).reshape(shape[:-1]),
            'mass_lod': np.where(inside, (a(g) * (smag[1] + smag[0])).sum(-1), 0.0).reshape(shape[:-1])}
