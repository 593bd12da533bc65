"""The restatement `dirt_amd.shading.shade_gbuffer_ibl` is checked against: `dirt_amd.lighting.image_based_lighting` on CPU
tensors, the mask composite and the clamp of DESIGN.md §7b, gradients by torch's autograd.  Every parameter is expanded to one
row per pixel and made a leaf: a parameter's gradient is the sum of its leaf's rows.  Run in float64 it is the reference; run in
float32 it is the composition users had before the kernel, whose error sets the tolerance (`measure_f32`).

`terms` writes the lighting out once more, term by term (the diffuse term, the specular term, the background), from the cube
look-ups of dirt_amd/texture.py; it is what the masses are taken of, what the deliberate mistakes of the sensitivity test are
made in, and `tests/test_shade_ibl.py` holds it against `image_based_lighting` itself.  The L1 mass of an element is taken per
term, per output channel and, at every normalisation x / max(|x|, 1e-12), per autograd path: the norm is taken of a detached
leaf copy of x, so the half of the gradient that flows through the norm and the direct half, which cancel along x, are added
by their absolute values (`_path_masses` of tests/shade_pbr_reference.py carries what arrives at the copy on).  A texel of a
cube collects one product per pixel and channel, whose sign is grad_out's (every other factor is >= 0 for an intensity, an
albedo and a mask >= 0 and S in [0, 1]): its mass is its gradient with |grad_out| in place of grad_out.

The table reference integrates A and B by the product midpoint rule in (u, phi) after the substitution u = the distribution
function of D nh, which flattens D -- equal cells in u, where `lighting.environment_brdf` takes equal cells in log(u / (1 - u)).

    python -m tests.shade_ibl_reference      # prints the float32 figures and the table reference's convergence, which the
                                             # constants of tests/test_shade_ibl.py restate
"""
import functools

import numpy as np
import torch

from dirt_amd import lighting
from dirt_amd.texture import directions_to_cube_indices, sample_cube
from tests.shade_pbr_reference import _path_masses
from tests.shade_reference import worst_ratio

ATTRIBUTES = (('colors', 3), ('material', 2), ('normals', 3), ('positions', 3), ('mask', 1))
PARAMS = ('intensity', 'background', 'camera_position')
KINDS = ('pixels', 'd_colors', 'd_material', 'd_normals', 'd_positions', 'd_mask', 'd_params', 'd_specular', 'd_irradiance')
MISTAKES = ('reflect_clamped', 'lod_from_r', 'swap_ab', 'drop_one_minus_s', 'no_half_texel')
MARGIN = 1.e-3          # the distance every drawn pixel keeps from every kink
MAX_REDRAWN = 0.05      # the share of a first draw that may lie nearer


# ---- the table

def table_reference(nv, rho, nu, nphi):
    """(A, B) at the points (nv, rho) (arrays of one shape), float64: the midpoint rule on nu x nphi equal cells of (u, phi),
    cos^2 theta_h = (1 - u) / (1 + (a2 - 1) u), phi over the full circle."""
    nv, rho = np.broadcast_arrays(np.asarray(nv, np.float64), np.asarray(rho, np.float64))
    out = np.empty(nv.shape + (2,))
    u = ((np.arange(nu) + 0.5) / nu)[:, None]
    phi = ((np.arange(nphi) + 0.5) / nphi * 2. * np.pi)[None, :]
    for at in np.ndindex(nv.shape):
        c, r = nv[at], rho[at]
        a2 = r ** 4
        k = (r + 1.) ** 2 / 8.
        cos2 = (1. - u) / (1. + (a2 - 1.) * u)
        nh = np.sqrt(cos2)
        h = np.stack(np.broadcast_arrays(np.sqrt(1. - cos2) * np.cos(phi), np.sqrt(1. - cos2) * np.sin(phi), nh), -1)
        v = np.array([np.sqrt(1. - c * c), 0., c])
        vh = h @ v
        l = 2. * vh[..., None] * h - v
        nl = l[..., 2]
        lit = (vh > 0) & (nl > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            w = np.where(lit, nl * vh / (nh * (nl * (1. - k) + k) * (c * (1. - k) + k)), 0.)   # D Vis nl over the density D nh / (4 vh)
        fc = (1. - vh) ** 5
        out[at] = (w * (1. - fc)).mean(), (w * fc).mean()
    return out


def table_points():
    """(nv, rho, (table size, row, column)) of the texels the table test looks at: every texel of a 4 x 4 table, and of the
    32 x 32 one the corners and the middle of its first and last rows (the narrowest lobe, the widest)."""
    at = [(4, i, j) for i in range(4) for j in range(4)] + [(32, i, j) for i in (0, 31) for j in (0, 15, 31)]
    return np.array([(j + 0.5) / s for s, i, j in at]), np.array([(i + 0.5) / s for s, i, j in at]), at


def table_reference_with_error(resolutions=((2048, 128), (4096, 256))):
    """-> (the reference at the finer resolution [points, 2], its convergence error: the largest difference between the two)"""
    nv, rho, _ = table_points()
    coarse, fine = (table_reference(nv, rho, *res) for res in resolutions)
    return fine, float(np.abs(fine - coarse).max())


@functools.lru_cache(maxsize=None)
def brdf_table(size):
    return lighting.environment_brdf(size).numpy()


# ---- the environment of a case

class Environment:
    """levels: L float32 arrays [6, n_k, n_k, 3], n_k = N >> k (each its own noise: the look-up does not care what filtered
    them); irradiance [6, M, M, 3]; table [S, S, 2]"""

    def __init__(self, rng, size, levels, irradiance_size, table_size):
        assert levels >= 1 and (size >> (levels - 1)) << (levels - 1) == size
        self.size, self.irradiance_size, self.table_size = size, irradiance_size, table_size
        self.levels = [rng.uniform(0.05, 1., (6, size >> k, size >> k, 3)).astype(np.float32) for k in range(levels)]
        self.irradiance = rng.uniform(0.05, 1., (6, irradiance_size, irradiance_size, 3)).astype(np.float32)
        self.table = brdf_table(table_size)

    def packed(self, levels=None):
        """[6, floats]: the levels as a `CubePyramid` packs them"""
        return np.concatenate([lv.reshape(6, -1) for lv in (self.levels if levels is None else levels)], 1)


# ---- the lighting, term by term

def _t(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)).to(dtype)


def _bilinear(table, row, col):
    s = table.shape[0]
    fr0, fc0 = torch.floor(row), torch.floor(col)
    fr, fc = (row - fr0)[:, None], (col - fc0)[:, None]
    r, c = fr0.long(), fc0.long()
    tap = lambda a, b: table[a.clamp(0, s - 1), b.clamp(0, s - 1)]   # noqa: E731
    return tap(r, c) * (1. - fc) * (1. - fr) + tap(r, c + 1) * fc * (1. - fr) + tap(r + 1, c) * (1. - fc) * fr + tap(r + 1, c + 1) * fc * fr


def _look(cube, d):
    return sample_cube(cube, *directions_to_cube_indices(d, int(cube.shape[1])))


def terms(p, n, c, r, mu, m, cam, intensity, background, levels, irradiance, table, min_roughness, f0, normalize, mistake=None):
    """p, n, c [V, 3]; r, mu [V]; m [V, 1]; cam, intensity, background [V, 3] -> ([diffuse, specular, background term] [V, 3]
    each: they add up to a pixel before the clamp, and what `kink_distance` reads)"""
    N, v = normalize(n), normalize(cam - p)
    nv_raw = (N * v).sum(-1)
    nv = nv_raw.clamp(min=0.)
    rho = r.clamp(min_roughness, 1.)
    F0 = f0 * (1. - mu)[:, None] + c * mu[:, None]
    R = (2. * (nv if mistake == 'reflect_clamped' else nv_raw))[:, None] * N - v
    S = int(table.shape[0])
    half = 0. if mistake == 'no_half_texel' else 0.5
    ab = _bilinear(table, (rho * S - half).clamp(0., S - 1.), (nv * S - half).clamp(0., S - 1.))
    A, B = (ab[:, 1:], ab[:, :1]) if mistake == 'swap_ab' else (ab[:, :1], ab[:, 1:])
    Sj = F0 * A + B
    top = len(levels) - 1
    lam = ((r if mistake == 'lod_from_r' else rho) * top).clamp(0., float(top))
    low = torch.floor(lam)
    f = (lam - low)[:, None]
    l0 = low.long()
    l1 = (l0 + 1).clamp(max=top)
    looked = torch.stack([_look(lv, R) for lv in levels])
    pick = lambda l: torch.gather(looked, 0, l[None, :, None].expand(1, -1, 3))[0]   # noqa: E731
    spec = (1. - f) * pick(l0) + f * pick(l1)
    E = _look(irradiance, n)
    wd = ((1. - mu)[:, None] if mistake == 'drop_one_minus_s' else (1. - Sj) * (1. - mu)[:, None]) * c
    info = dict(R=R.detach(), nv_raw=nv_raw.detach(), lam=(rho * top).detach())
    return [(intensity * (wd * E)) * m, (intensity * (Sj * spec)) * m, background * (1. - m)], info


def _plain_normalize(x):
    return torch.nn.functional.normalize(x, dim=-1, eps=1.e-12)


def compose(gbuffer, env, layout, colors=None, material=None, intensity=(1., 1., 1.), camera_position=(0., 0., 4.),
            background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04, grad_out=None, scene_index=None,
            dtype=torch.float64, masses=True, mistake=None):
    """gbuffer [N, Cg] (float32 values); env: an `Environment`; intensity, camera_position, background [3] or [R, 3] with
    scene_index [N] (pixel -> row); layout: first channels of colors, material, normals, positions, mask (colors / material
    absent with `colors` [N, 3] / `material` [N, 2] given; mask may be None).  mistake: one of MISTAKES, made in `terms`.
    -> dict: out, pre, and what `kink_distance` reads; with grad_out [N, 3] also d_gbuffer, d_<attribute> ([N, 0] for an absent
    mask), d_params {name: [R, 3]}, d_specular [6, floats], d_irradiance; with masses also mass_out and mass_<each of those>."""
    g = _t(gbuffer, dtype).requires_grad_(True)
    n_px = g.shape[0]
    idx = torch.zeros(n_px, dtype=torch.long) if scene_index is None else torch.as_tensor(np.asarray(scene_index)).long()
    col = _t(colors, dtype).requires_grad_(True) if colors is not None else None
    mat = _t(material, dtype).requires_grad_(True) if material is not None else None
    shared = {k: _t(v, dtype).reshape(-1, 3) for k, v in zip(PARAMS, (intensity, background, camera_position))}
    at = lambda r: idx if r.shape[0] > 1 else torch.zeros_like(idx)   # noqa: E731
    leaves = {k: r[at(r)].clone().requires_grad_(True) for k, r in shared.items()}
    levels = [_t(lv, dtype).requires_grad_(True) for lv in env.levels]
    irr = _t(env.irradiance, dtype).requires_grad_(True)
    table = _t(env.table, dtype)
    has_mask = layout.get('mask') is not None

    def parts(gb, cl, mt):
        sl = lambda k, w: gb[:, layout[k]:layout[k] + w]   # noqa: E731
        c = cl if cl is not None else sl('colors', 3)
        rm = mt if mt is not None else sl('material', 2)
        m = sl('mask', 1) if has_mask else torch.ones(n_px, 1, dtype=dtype)
        return c, rm[:, 0], rm[:, 1], sl('normals', 3), sl('positions', 3), m

    def all_terms(gb, cl, mt, lv, lvls, ir, normalize):
        c, r, mu, n, p, m = parts(gb, cl, mt)
        return terms(p, n, c, r, mu, m, lv['camera_position'], lv['intensity'], lv['background'], lvls, ir, table, min_roughness,
                     dielectric_f0, normalize, mistake)

    # ---- values and gradients: lighting.image_based_lighting itself
    c, r, mu, n, p, m = parts(g, col, mat)
    qs, info = all_terms(g, col, mat, leaves, levels, irr, _plain_normalize)
    if mistake is None:
        lit = lighting.image_based_lighting(p[:, None], n[:, None], c[:, None], r[:, None], mu[:, None], leaves['camera_position'], levels, irr,
                                            table, leaves['intensity'], min_roughness, dielectric_f0)[:, 0]
        pre = lit * m + leaves['background'] * (1. - m)
    else:
        pre = sum(qs)
    out = torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre
    res = {'out': out.detach(), 'pre': pre.detach(), 'roughness': r.detach(), 'normals': n.detach(), 'terms': [q.detach() for q in qs]}
    res.update(info)

    def split(d_g, d_col, d_mat, prefix):
        d = {prefix + 'gbuffer': d_g}
        for k, w in ATTRIBUTES:
            if k == 'colors' and col is not None:
                d[prefix + k] = d_col
            elif k == 'material' and mat is not None:
                d[prefix + k] = d_mat
            elif k == 'mask' and not has_mask:
                d[prefix + k] = d_g[:, 0:0]
            else:
                d[prefix + k] = d_g[:, layout[k]:layout[k] + w]
        return d

    zero = lambda like, x: torch.zeros_like(like) if x is None else x   # noqa: E731
    pack = lambda per_level: torch.cat([x.reshape(6, -1) for x in per_level], 1)   # noqa: E731
    n_lv = len(levels)
    if grad_out is not None:
        go = _t(grad_out, dtype)
        inputs = [g] + [leaves[k] for k in PARAMS] + levels + [irr] + [x for x in (col, mat) if x is not None]
        grads = [zero(x, gr) for x, gr in zip(inputs, torch.autograd.grad((out * go).sum(), inputs, allow_unused=True))]
        extra = grads[5 + n_lv:]
        res.update(split(grads[0], extra[0] if col is not None else None, extra[-1] if mat is not None else None, 'd_'))
        res['d_params'] = {k: torch.zeros_like(shared[k]).index_add_(0, at(shared[k]), gr) for k, gr in zip(PARAMS, grads[1:4])}
        res['d_specular'], res['d_irradiance'] = pack(grads[4:4 + n_lv]), grads[4 + n_lv]
    if not masses:
        return res

    # ---- L1 masses: every term, output channel and autograd path apart
    res['mass_out'] = sum(q.detach().abs() for q in qs)
    if grad_out is None:
        return res
    gm = g.detach().clone().requires_grad_(True)
    cm = col.detach().clone().requires_grad_(True) if col is not None else None
    mm = mat.detach().clone().requires_grad_(True) if mat is not None else None
    lm = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    lvm = [x.detach().clone().requires_grad_(True) for x in levels]
    irm = irr.detach().clone().requires_grad_(True)
    cuts = []

    def cut_normalize(x):
        leaf = x.detach().requires_grad_(True)
        cuts.append((leaf, x))
        return x / torch.linalg.vector_norm(leaf, dim=-1, keepdim=True).clamp_min(1.e-12)

    qm, _ = all_terms(gm, cm, mm, lm, lvm, irm, cut_normalize)
    gate = ((pre >= clamp[0]) & (pre <= clamp[1])).to(dtype).detach() if clamp is not None else torch.ones_like(pre).detach()
    inputs = [gm] + [lm[k] for k in PARAMS] + [x for x in (cm, mm) if x is not None]
    mass = [torch.zeros_like(x) for x in inputs]
    for q in qm:
        for j in range(3):
            _path_masses((gate[:, j] * go[:, j] * q[:, j]).sum(), None, inputs, cuts, mass)
    extra = mass[4:]
    res.update(split(mass[0], extra[0] if cm is not None else None, extra[-1] if mm is not None else None, 'mass_'))
    res['mass_params'] = {k: torch.zeros_like(shared[k]).index_add_(0, at(shared[k]), ms) for k, ms in zip(PARAMS, mass[1:4])}
    cube_mass = torch.autograd.grad(((gate * go.abs()) * (qm[0] + qm[1])).sum(), lvm + [irm], allow_unused=True)
    cube_mass = [zero(x, gr).abs() for x, gr in zip(lvm + [irm], cube_mass)]
    res['mass_specular'], res['mass_irradiance'] = pack(cube_mass[:n_lv]), cube_mass[n_lv]
    return res


# ---- the kinks

def _index_distance(x, n):
    """the distance of the unclamped index x at a level of size n from where its taps or its clamp change"""
    inside = np.abs(x - np.round(x))
    return np.where(x < 0., -x, np.where(x > n - 1., x - (n - 1.), inside))


def _cube_distance(d, sizes):
    """d [V, 3] float64 directions, sizes [V, K] the level sizes looked up -> [V]: the least distance, in index units, of the look-ups from
    a tap-lattice line, and the relative gap of the two largest components (a face tie)"""
    d = np.asarray(d, np.float64)
    valid = np.isfinite(d).all(1) & (np.abs(d).max(1) > 0)
    a = np.sort(np.abs(d), 1)
    tie = (a[:, 2] - a[:, 1]) / np.where(a[:, 2] > 0, a[:, 2], 1.)
    # (sc / a, tc / a) before any clamp, by the face rule of dirt_texture_cube.hip (spec 3)
    x, y, z = d.T
    ax, ay, az = np.abs(d).T
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    major = np.where(is_x, x, np.where(is_y, y, z))
    pos = major > 0
    sc = np.where(is_x, np.where(pos, -z, z), np.where(is_y, x, np.where(pos, x, -x)))
    tc = np.where(is_y, np.where(pos, z, -z), -y)
    am = np.where(np.abs(major) > 0, np.abs(major), 1.)
    dist = tie
    for k in range(sizes.shape[1]):
        nk = sizes[:, k].astype(np.float64)
        for s in (sc / am, tc / am):
            dist = np.minimum(dist, _index_distance((s + 1.) * 0.5 * nk - 0.5, nk))
    return np.where(valid, dist, np.inf)   # an invalid direction looks nothing up


def kink_distance(res, env, clamp, min_roughness):
    """[N]: how near each pixel of `compose`'s result comes to a kink (the module's docstring of tests/test_shade_ibl.py lists them)"""
    r = res['roughness'].numpy().astype(np.float64)
    rho = np.clip(r, min_roughness, 1.)
    L, S = len(env.levels), env.table_size
    lam = rho * (L - 1)
    l0 = np.floor(lam).astype(int)
    l1 = np.minimum(l0 + 1, L - 1)
    dist = np.minimum(np.abs(r - min_roughness), np.abs(r - 1.))
    nv_raw = res['nv_raw'].numpy()
    dist = np.minimum(dist, np.abs(nv_raw))
    if L > 1:
        dist = np.minimum(dist, np.abs(lam - np.round(lam)))
    dist = np.minimum(dist, _cube_distance(res['R'].numpy(), np.stack([env.size >> l0, env.size >> l1], 1)))
    dist = np.minimum(dist, _cube_distance(res['normals'].numpy(), np.full((len(r), 1), env.irradiance_size)))
    for x in (np.maximum(nv_raw, 0.), rho):
        dist = np.minimum(dist, _index_distance(x * S - 0.5, float(S)))
    if clamp is not None:
        pre = res['pre'].numpy()
        dist = np.minimum(dist, np.minimum(np.abs(pre - clamp[0]), np.abs(pre - clamp[1])).min(1))
    return dist


def random_pixels(rng, n, cg, layout, min_roughness=0.04, covered=0.7):
    """(gbuffer [n, cg], colors [n, 3] or None, material [n, 2] or None): albedo U(0.05, 0.95), unit normals scaled by
    U(0.8, 1.2), positions in [-1, 1]^3, roughness inside (min_roughness, 1), metalness U(0, 1), a mask of 0 / 1 / fractional
    coverage (70 % / 10 % fractional); the channels no attribute uses hold noise."""
    g = rng.standard_normal((n, cg)).astype(np.float32)
    col = rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)
    lo, hi = min_roughness + 0.01, 0.99
    mat = np.stack([rng.uniform(lo, hi, n), rng.uniform(0., 1., n)], 1).astype(np.float32)
    if 'colors' in layout:
        g[:, layout['colors']:layout['colors'] + 3] = col
    if 'material' in layout:
        g[:, layout['material']:layout['material'] + 2] = mat
    nn = rng.standard_normal((n, 3))
    g[:, layout['normals']:layout['normals'] + 3] = nn / np.linalg.norm(nn, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (n, 1))
    g[:, layout['positions']:layout['positions'] + 3] = rng.uniform(-1., 1., (n, 3))
    if layout.get('mask') is not None:
        u = rng.uniform(0., 1., n)
        g[:, layout['mask']] = np.where(u < covered, 1., np.where(u < covered + 0.1, rng.uniform(0.1, 0.9, n), 0.))
    return g, (None if 'colors' in layout else col), (None if 'material' in layout else mat)


def draw_off_kinks(rng, n, cg, layout, env, kw, scene_index=None, fix=None):
    """Random pixels that all stay MARGIN off the kinks: draw, judge by the float64 restatement alone, redraw the pixels it places
    nearer.  The share redrawn from the first draw must stay under MAX_REDRAWN (of 64 pixels or more: one pixel of three is a third).  fix(g, rows): a case's own placement of the
    pixels `rows` (normals and positions that send every look-up to one face, ...), applied to every draw.
    -> (gbuffer, colors or None, material or None, share)"""
    mr = kw.get('min_roughness', 0.04)
    g, col, mat = random_pixels(rng, n, cg, layout, mr)
    if fix is not None:
        fix(g, np.arange(n))
    share = None
    for _ in range(30):
        ref = compose(g, env, layout, colors=col, material=mat, scene_index=scene_index, masses=False, **kw)
        bad = kink_distance(ref, env, kw.get('clamp', (0., 1.)), mr) < MARGIN
        if share is None:
            share = float(bad.mean())
            assert share < MAX_REDRAWN or n < 64, 'share of redrawn pixels %.3f' % share
        if not bad.any():
            return g, col, mat, share
        g[bad], c2, m2 = random_pixels(rng, int(bad.sum()), cg, layout, mr)
        if fix is not None:
            fix(g, np.flatnonzero(bad))
        if col is not None:
            col[bad] = c2
        if mat is not None:
            mat[bad] = m2
    raise AssertionError('could not draw pixels off the kinks')


# ---- the comparison

PAIRS = (('pixels', 'out', 'mass_out'),) + tuple(('d_' + k, 'd_' + k, 'mass_' + k) for k, _ in ATTRIBUTES) + \
    (('d_specular', 'd_specular', 'mass_specular'), ('d_irradiance', 'd_irradiance', 'mass_irradiance'))


def ratios(got, ref):
    """The worst |got - ref| / mass per kind of result; got: dict with out, d_<attribute>, d_specular, d_irradiance, d_params
    {name: tensor} (entries that are missing or None are skipped), ref: `compose(..., masses=True)`."""
    worst = {}
    as64 = lambda x: np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)   # noqa: E731
    for kind, key, mass in PAIRS:
        if got.get(key) is not None and key in ref:
            worst[kind] = worst_ratio(as64(got[key]).reshape(ref[key].shape), ref[key].numpy(), ref[mass].numpy())
    for k, v in (got.get('d_params') or {}).items():
        if v is not None:
            worst['d_params'] = max(worst.get('d_params', 0.), worst_ratio(as64(v).reshape(ref['d_params'][k].shape), ref['d_params'][k].numpy(),
                                                                           ref['mass_params'][k].numpy()))
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
    from tests import test_shade_ibl
    print({k: '%.3e' % v for k, v in measure_f32(c.measure() for c in test_shade_ibl.tolerance_cases().values()).items()})
    print('table reference: convergence error %.3e' % table_reference_with_error()[1])
