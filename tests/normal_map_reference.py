"""The restatements `dirt_amd.geometry.vertex_tangents` and `dirt_amd.shading.perturb_normals` (and their torch forms in
`dirt_amd.lighting`) are checked against: the specification of DESIGN.md §7g written out in numpy float64, forward and
backward, every step by hand -- no autograd, so that it shares no code with `dirt_amd.lighting` (tests/test_normal_map.py
checks that torch's autograd of the float64 torch form agrees with it to 1e-12 of the masses).

Every value travels with the L1 mass of its terms (`VM`): a sum's mass is the sum of its terms' masses, a product's the
product, a normalisation's the first-order propagation |d u_j| <= m_j / |v| + |u_j| sum_k |u_k| m_k / |v|.  The mass of an
input is its absolute value.  An element whose mass is zero must be exact.

The float32 torch composition run on the same inputs is what users had before the kernels; its worst |f32 - ref64| / mass
per kind of result sets the tolerance (`measure_f32`):

    python -m tests.normal_map_reference      # prints the float32 figures the constants of tests/test_normal_map.py restate
"""
import numpy as np
import torch

from tests.shade_reference import worst_ratio

KINDS = ('tangents', 'd_vertices', 'd_normals', 'out', 'd_gbuffer', 'd_normal_map')
MARGIN = 0.05       # |det| and |cross(n, t) . Bt|: at least this share of their terms' mass
MIN_SIN = 0.3       # between a tangent (sum) and the normal
MIN_Z = 0.5         # of the decoded normal-map vector


class VM:
    """a float64 array and, per element, the L1 mass of the terms it was added up from"""

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=np.float64)

    def __add__(self, o):
        return VM(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        return VM(self.v - o.v, self.m + o.m)

    def __neg__(self):
        return VM(-self.v, self.m)

    def __mul__(self, o):
        if isinstance(o, VM):
            return VM(self.v * o.v, self.m * o.m)
        return VM(self.v * o, self.m * np.abs(o))     # an exact factor

    def __getitem__(self, k):
        return VM(self.v[k], self.m[k])

    def where(self, ok, other):
        return VM(np.where(ok, self.v, other.v), np.where(ok, self.m, other.m))


def dot(a, b):
    p = a * b
    return VM(p.v.sum(-1, keepdims=True), p.m.sum(-1, keepdims=True))


def cross(a, b):
    c = [a[..., (j + 1) % 3:(j + 1) % 3 + 1] * b[..., (j + 2) % 3:(j + 2) % 3 + 1] - a[..., (j + 2) % 3:(j + 2) % 3 + 1] * b[..., (j + 1) % 3:(j + 1) % 3 + 1]
         for j in range(3)]
    return VM(np.concatenate([x.v for x in c], -1), np.concatenate([x.m for x in c], -1))


def over(a, length):
    """a / length, the length taken as exact"""
    return VM(a.v / length, a.m / length)


def unit(a):
    """-> (a / |a| with its mass, |a| (1 where a is zero), a . a > 0)"""
    aa = (a.v * a.v).sum(-1, keepdims=True)
    ok = aa > 0
    length = np.sqrt(np.where(ok, aa, 1.))
    u = a.v / length
    return VM(u, a.m / length + np.abs(u) * (np.abs(u) * a.m).sum(-1, keepdims=True) / length), length, ok


def scatter(values, index, rows):
    """sum of values[f] into row index[f]"""
    out_v, out_m = np.zeros((rows,) + values.v.shape[1:]), np.zeros((rows,) + values.v.shape[1:])
    np.add.at(out_v, index, values.v)
    np.add.at(out_m, index, values.m)
    return VM(out_v, out_m)


def _f64(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def _face_coefficients(uvs, faces):
    uv = _f64(uvs)
    with np.errstate(invalid='ignore'):
        d1, d2 = uv[faces[:, 1]] - uv[faces[:, 0]], uv[faces[:, 2]] - uv[faces[:, 0]]
        du1, dv1, du2, dv2 = d1[:, 0:1], d1[:, 1:2], d2[:, 0:1], d2[:, 1:2]
        det = du1 * dv2 - du2 * dv1
        live = np.isfinite(det) & (det != 0)     # a dead face: the four coefficients exactly 0, whatever its uvs hold
        a, b, c, d = (np.where(live, np.sign(det) * x, 0.) for x in (dv2, dv1, du1, du2))
        share = np.where(live, np.abs(det) / np.maximum(np.abs(du1 * dv2) + np.abs(du2 * dv1), 1e-300), 0.)
    return a, b, c, d, share[:, 0]


def tangents(vertices, normals, uvs, faces, grad_out=None):
    """One scene: vertices [V, 3|4], normals [V, 3], uvs [V, 2], faces [F, 3] (float32 values) -> dict: tangents [V, 4] and
    mass_tangents; det_share [F], w_share [V], sin [V] (what the draws are rejected by); with grad_out [V, 4] also d_vertices
    [V, 3|4], d_normals [V, 3] and their masses."""
    p, n = VM(_f64(vertices)[:, :3]), VM(_f64(normals))
    faces = np.asarray(faces, dtype=np.int64)
    V, C = p.v.shape[0], np.asarray(vertices).shape[-1]
    a, b, c, d, det_share = _face_coefficients(uvs, faces)
    p0, p1, p2 = (p[faces[:, k]] for k in range(3))
    e1, e2 = VM(p1.v - p0.v), VM(p2.v - p0.v)     # (the difference of two float32 values is rounded once, relative to itself: a term of its own)
    t_f, b_f = e1 * a - e2 * b, e2 * c - e1 * d
    T, Bt = VM(np.zeros((V, 3))), VM(np.zeros((V, 3)))
    for k in range(3):
        T, Bt = T + scatter(t_f, faces[:, k], V), Bt + scatter(b_f, faces[:, k], V)
    nt = dot(n, T)
    x = T - n * nt
    t, length, ok = unit(x)
    t = t.where(ok, VM(np.zeros((V, 3))))
    c = cross(n, t)
    side = dot(c, Bt)
    w = np.where(side.v < 0, -1., 1.)
    side_mass = (np.abs(c.v) * Bt.m).sum(-1)     # of the sign's terms: the faces' b_f, each weighed by the direction it is measured along
    lenT = np.sqrt((T.v * T.v).sum(-1))
    res = {'tangents': np.concatenate([t.v, w], -1), 'mass_tangents': np.concatenate([t.m, np.zeros((V, 1))], -1),
           'det_share': det_share, 'w_share': np.where(ok[:, 0], np.abs(side.v[:, 0]) / np.maximum(side_mass, 1e-300), 1.),
           'sin': np.where(lenT > 0, length[:, 0] / np.maximum(lenT, 1e-300), 1.), 'valid': ok[:, 0]}
    if grad_out is None:
        return res
    gt = VM(_f64(grad_out)[:, :3])
    zero = VM(np.zeros((V, 3)))
    gx = over(gt - t * dot(t, gt), length)
    ng = dot(n, gx)
    GT = (gx - n * ng).where(ok, zero)
    dn = (-(gx * nt + T * ng)).where(ok, zero)
    Gf = GT[faces[:, 0]] + GT[faces[:, 1]] + GT[faces[:, 2]]
    dp = scatter(Gf * b - Gf * a, faces[:, 0], V) + scatter(Gf * a, faces[:, 1], V) + scatter(-(Gf * b), faces[:, 2], V)
    pad = np.zeros((V, C - 3))
    res.update(d_vertices=np.concatenate([dp.v, pad], -1), mass_d_vertices=np.concatenate([dp.m, pad], -1), d_normals=dn.v, mass_d_normals=dn.m)
    return res


def perturb(normals, tangents4, normal_map, strength=1., encoded=True, grad_out=None):
    """[N, 3], [N, 4], [N, 3] (float32 values) -> dict: out [N, 3], mass_out, valid [N], sin [N] (tangent against normal), z [N]
    (decoded); with grad_out [N, 3] also d_normals [N, 3], d_tangents [N, 4], d_normal_map [N, 3] and their masses."""
    n, tw, m = VM(_f64(normals)), VM(_f64(tangents4)), VM(_f64(normal_map))
    t, w = tw[:, :3], tw[:, 3:4]
    d = (m * 2. - VM(np.ones_like(m.v))) if encoded else m
    scale = np.array([float(strength), float(strength), 1.])
    d = d * scale
    N, ln, ok_n = unit(n)
    s = dot(N, t)
    x = t - N * s
    T, lx, ok_x = unit(x)
    C = cross(N, T)
    Bv = C * w
    y = (T * d[:, 0:1] + Bv * d[:, 1:2]) + N * d[:, 2:3]
    o, ly, ok_y = unit(y)
    ok = ok_n & ok_x & ok_y
    out = o.where(ok, n)
    lt = np.sqrt((t.v * t.v).sum(-1))
    res = {'out': out.v, 'mass_out': out.m, 'valid': ok[:, 0], 'sin': np.where(lt > 0, lx[:, 0] / np.maximum(lt, 1e-300), 0.), 'z': d.v[:, 2]}
    if grad_out is None:
        return res
    g = VM(_f64(grad_out))
    zero = VM(np.zeros_like(n.v))
    gy = over(g - o * dot(o, g), ly)
    gd = VM(np.concatenate([dot(gy, T).v, dot(gy, Bv).v, dot(gy, N).v], -1), np.concatenate([dot(gy, T).m, dot(gy, Bv).m, dot(gy, N).m], -1))
    gw = dot(gy, C) * d[:, 1:2]
    gC = gy * (w * d[:, 1:2])
    gT = gy * d[:, 0:1] + cross(gC, N)
    gx = over(gT - T * dot(T, gT), lx)
    ngx = dot(N, gx)
    gt = gx - N * ngx
    gN = (gy * d[:, 2:3] + cross(T, gC)) - (gx * s + t * ngx)
    gn = over(gN - N * dot(N, gN), ln)
    gm = gd * (scale * (2. if encoded else 1.))
    gn, gt, gw, gm = gn.where(ok, g), gt.where(ok, zero), gw.where(ok, zero[:, :1]), gm.where(ok, zero)
    res.update(d_normals=gn.v, mass_d_normals=gn.m, d_tangents=np.concatenate([gt.v, gw.v], -1), mass_d_tangents=np.concatenate([gt.m, gw.m], -1),
               d_normal_map=gm.v, mass_d_normal_map=gm.m)
    return res


def perturb_gbuffer(gbuffer, normal_map, on, ot, strength=1., encoded=True, grad_out=None):
    """`perturb` on a G-buffer [N, Cg] with the normals at channel `on` and the tangents at `ot`, as `shading.perturb_normals`
    returns it: out [N, Cg] (the other channels copied, mass = |value|); with grad_out [N, Cg] d_gbuffer [N, Cg] (grad_out
    passed through, the normal channels replaced, the tangent channels added to) and d_normal_map [N, 3], with masses."""
    g = _f64(gbuffer)
    go = None if grad_out is None else _f64(grad_out)
    r = perturb(g[:, on:on + 3], g[:, ot:ot + 4], normal_map, strength, encoded, None if go is None else go[:, on:on + 3])
    out, mass = g.copy(), np.abs(g)
    out[:, on:on + 3], mass[:, on:on + 3] = r['out'], r['mass_out']
    res = {'out': out, 'mass_out': mass, 'valid': r['valid'], 'sin': r['sin'], 'z': r['z']}
    if go is not None:
        dg, dm = go.copy(), np.abs(go)
        dg[:, on:on + 3], dm[:, on:on + 3] = r['d_normals'], r['mass_d_normals']
        dg[:, ot:ot + 4] += r['d_tangents']
        dm[:, ot:ot + 4] += r['mass_d_tangents']
        res.update(d_gbuffer=dg, mass_d_gbuffer=dm, d_normal_map=r['d_normal_map'], mass_d_normal_map=r['mass_d_normal_map'])
    return res


# ---- the torch forms on the CPU, in either precision

def torch_tangents(vertices, normals, uvs, faces, grad_out, dtype):
    from dirt_amd import lighting
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float32)).to(dtype).requires_grad_(True)
    n = torch.as_tensor(np.asarray(normals, dtype=np.float32)).to(dtype).requires_grad_(True)
    out = lighting.vertex_tangents(v, n, torch.as_tensor(np.asarray(uvs, dtype=np.float32)).to(dtype), torch.as_tensor(np.asarray(faces)).long())
    out.backward(torch.as_tensor(np.asarray(grad_out, dtype=np.float32)).to(dtype))
    return {'tangents': out.detach().numpy(), 'd_vertices': v.grad.numpy(), 'd_normals': n.grad.numpy()}


def torch_perturb_gbuffer(gbuffer, normal_map, on, ot, strength, encoded, grad_out, dtype):
    """the route users had: `lighting.perturb_normals` on slices and a `torch.cat` back into the G-buffer"""
    from dirt_amd import lighting
    g = torch.as_tensor(np.asarray(gbuffer, dtype=np.float32)).to(dtype).requires_grad_(True)
    m = torch.as_tensor(np.asarray(normal_map, dtype=np.float32)).to(dtype).requires_grad_(True)
    new = lighting.perturb_normals(g[:, on:on + 3], g[:, ot:ot + 4], m, strength=strength, encoded=encoded)
    out = torch.cat([g[:, :on], new, g[:, on + 3:]], dim=1)
    out.backward(torch.as_tensor(np.asarray(grad_out, dtype=np.float32)).to(dtype))
    return {'out': out.detach().numpy(), 'd_gbuffer': g.grad.numpy(), 'd_normal_map': m.grad.numpy()}


def ratios(got, ref, kinds):
    """The worst |got - ref| / mass per kind of result in `kinds` ((kind, key) pairs; `ref` holds key and mass_<key>)."""
    return {kind: worst_ratio(_f64(got[key]).reshape(ref[key].shape), ref[key], ref['mass_' + key]) for kind, key in kinds if got.get(key) is not None}


TANGENT_KINDS = (('tangents', 'tangents'), ('d_vertices', 'd_vertices'), ('d_normals', 'd_normals'))
PIXEL_KINDS = (('out', 'out'), ('d_gbuffer', 'd_gbuffer'), ('d_normal_map', 'd_normal_map'))


def measure_f32(mesh_cases, pixel_cases):
    """mesh_cases: iterable of (vertices, normals, uvs, faces, grad_out) per scene; pixel_cases: of (gbuffer, normal_map, on, ot,
    strength, encoded, grad_out) -> the worst |f32 - ref64| / mass of the float32 torch composition per kind of result (KINDS)."""
    worst = dict.fromkeys(KINDS, 0.)
    for v, n, uv, f, go in mesh_cases:
        for k, x in ratios(torch_tangents(v, n, uv, f, go, torch.float32), tangents(v, n, uv, f, go), TANGENT_KINDS).items():
            worst[k] = max(worst[k], x)
    for g, m, on, ot, strength, encoded, go in pixel_cases:
        r32 = torch_perturb_gbuffer(g, m, on, ot, strength, encoded, go, torch.float32)
        for k, x in ratios(r32, perturb_gbuffer(g, m, on, ot, strength, encoded, go), PIXEL_KINDS).items():
            worst[k] = max(worst[k], x)
    return worst


# ---- inputs off the discontinuities and away from ill-conditioned frames

def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def strip_mesh(V):
    """A zigzag triangle strip of V vertices in the plane: face i = (i, i + 1, i + 2), so F = V - 2 and a vertex has up to three faces."""
    i = np.arange(V)
    xy = np.stack([0.5 * i, (i % 2).astype(np.float64)], 1)
    return xy, np.stack([i[:-2], i[1:-1], i[2:]], 1).astype(np.int32)


def fan_mesh(rim, turns=12):
    """A fan of `rim` faces around vertex 0, the hub, whose list has `rim` entries.  The rim winds `turns` times around the hub
    on a growing radius, so that no face is a sliver: one of 300 faces in a single turn has an angle of 1.2 degrees at the
    hub, and a determinant of a fiftieth of its terms."""
    k = np.arange(rim)
    a = 2. * np.pi * turns * k / rim
    xy = np.concatenate([np.zeros((1, 2)), (1. + k / rim)[:, None] * np.stack([np.cos(a), np.sin(a)], 1)])
    return xy, np.stack([np.zeros(rim, np.int64), 1 + k, 1 + (k + 1) % rim], 1).astype(np.int32)


def cube_mesh():
    """A cube with split uv seams: four vertices per side, each side its own square of the uv atlas -> (positions [24, 3],
    unit normals [24, 3], uvs [24, 2], faces [12, 3])"""
    pos, nrm, uvs, faces = [], [], [], []
    for side in range(6):
        axis, sign = side % 3, 1. if side < 3 else -1.
        u_axis, v_axis = (axis + 1) % 3, (axis + 2) % 3
        for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = np.zeros(3)
            p[axis], p[u_axis], p[v_axis] = sign, (2 * cu - 1) * sign, 2 * cv - 1
            pos.append(p)
            nrm.append(np.eye(3)[axis] * sign)
            uvs.append([(side % 3 + cu * 0.9 + 0.05) / 3., (side // 3 + cv * 0.9 + 0.05) / 2.])
        faces += [[4 * side, 4 * side + 1, 4 * side + 2], [4 * side, 4 * side + 2, 4 * side + 3]]
    return np.array(pos), np.array(nrm), np.array(uvs), np.array(faces, dtype=np.int32)


def draw_mesh(rng, xy, faces, components=3, jitter=0.05, max_rejected=0.05):
    """A sheet over the plane points `xy` [V, 2]: positions (xy, a height) with jitter (`jitter` in the plane, four times that in
    height: a fraction of the shortest edge), uvs a rotated, scaled copy of xy with jitter, unit normals around +z.  Vertices of a face or with a frame too close to a discontinuity (MARGIN, MIN_SIN) are
    redrawn; the share redrawn after the first draw must stay under `max_rejected`.
    -> (vertices [V, components], normals, uvs, share), float32"""
    V = xy.shape[0]
    angle, scale = rng.uniform(0., 2. * np.pi), rng.uniform(0.05, 0.2)
    rot = scale * np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
    v, n, uv = np.zeros((V, components), np.float32), np.zeros((V, 3), np.float32), np.zeros((V, 2), np.float32)

    def fill(rows):
        k = len(rows)
        v[rows, :2] = xy[rows] + rng.normal(0., jitter, (k, 2))
        v[rows, 2] = rng.normal(0., 4. * jitter, k)
        if components == 4:
            v[rows, 3] = rng.uniform(0.5, 2., k)
        uv[rows] = xy[rows] @ rot + 0.5 + rng.normal(0., 0.4 * jitter * scale, (k, 2))
        n[rows] = _unit(np.array([0., 0., 1.]) + rng.normal(0., 0.3, (k, 3)))

    return v, n, uv, _redraw(fill, v, n, uv, faces, max_rejected)


def _redraw(fill, v, n, uv, faces, max_rejected):
    """The reject-and-redraw loop of the mesh draws: `fill(rows)` draws those rows of v, n, uv in place; the vertices of a face
    or with a frame too close to a discontinuity (MARGIN, MIN_SIN) are drawn again.  -> the share rejected from the first draw"""
    fill(np.arange(len(v)))
    share = None
    for _ in range(20):
        r = tangents(v, n, uv, faces)
        bad = (r['w_share'] < MARGIN) | (r['sin'] < MIN_SIN)
        bad[np.unique(faces[r['det_share'] < MARGIN])] = True
        if share is None:
            share = float(bad.mean())
            assert share < max_rejected, 'share of redrawn vertices %.3f' % share
        if not bad.any():
            return share
        fill(np.nonzero(bad)[0])
    raise AssertionError('could not draw a mesh off the discontinuities')


def torus_mesh(nu, nv, major=1., minor=0.4):
    """A torus as an (nu + 1) x (nv + 1) grid with both seams split (the last row and column repeat the first in space, with
    uvs of their own): vertex (i, j) has uv = (i / nu, j / nv), u around the axis and v around the tube; two faces per cell,
    so a vertex has 1 to 6 faces.  d p / d u x d p / d v points out of the tube: the handedness is +1 everywhere.
    -> (positions [V, 3], unit normals out of the tube [V, 3], uvs [V, 2], faces [2 nu nv, 3])"""
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij'))
    theta, phi = 2. * np.pi * i / nu, 2. * np.pi * j / nv
    nrm = np.stack([np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)], 1)
    pos = major * np.stack([np.cos(theta), np.sin(theta), np.zeros_like(theta)], 1) + minor * nrm
    ci, cj = (x.reshape(-1) for x in np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij'))
    at = lambda a, b: a * (nv + 1) + b   # noqa: E731
    faces = np.concatenate([np.stack([at(ci, cj), at(ci + 1, cj), at(ci + 1, cj + 1)], 1), np.stack([at(ci, cj), at(ci + 1, cj + 1), at(ci, cj + 1)], 1)])
    return pos, nrm, np.stack([i / nu, j / nv], 1), faces.astype(np.int32)


def draw_torus(rng, nu, nv, mirrored=False, components=3, max_rejected=0.05):
    """`torus_mesh` with jitter, through the reject-and-redraw loop of the sheets: positions by 5 % of the shortest edge, normals
    as the sheets' (a standard deviation of 0.3 per component, then unit), uvs by 2 % of a cell; mirrored: u -> 1 - u before the
    jitter, which turns the handedness to -1 everywhere.  -> (vertices [V, components], normals, uvs, faces, share), float32"""
    pos, nrm, uv0, faces = torus_mesh(nu, nv)
    if mirrored:
        uv0[:, 0] = 1. - uv0[:, 0]
    edges = np.concatenate([pos[faces[:, a]] - pos[faces[:, b]] for a, b in ((0, 1), (1, 2), (2, 0))])
    sigma = 0.05 * float(np.linalg.norm(edges, axis=1).min())
    V = len(pos)
    v, n, uv = np.zeros((V, components), np.float32), np.zeros((V, 3), np.float32), np.zeros((V, 2), np.float32)

    def fill(rows):
        k = len(rows)
        v[rows, :3] = pos[rows] + rng.normal(0., sigma, (k, 3))
        if components == 4:
            v[rows, 3] = rng.uniform(0.5, 2., k)
        uv[rows] = uv0[rows] + rng.normal(0., 0.02, (k, 2)) / np.array([nu, nv])
        n[rows] = _unit(nrm[rows] + rng.normal(0., 0.3, (k, 3)))

    return v, n, uv, faces, _redraw(fill, v, n, uv, faces, max_rejected)


def random_pixels(rng, n, cg, on, ot, encoded=True):
    """(gbuffer [n, cg], normal_map [n, 3]): normals standard-normal vectors (every second pixel: of unit length), tangents with
    half of their part along the normal removed, a handedness of -1 / +1 (a fifth: a fraction, as interpolation leaves it), a
    decoded map of x, y in [-1, 1] and z in [MIN_Z, 1]; the channels no attribute uses hold noise."""
    g = rng.standard_normal((n, cg)).astype(np.float32)
    nn = rng.standard_normal((n, 3))
    nn[::2] = _unit(nn[::2])
    N = _unit(nn)
    t = rng.standard_normal((n, 3))
    t -= 0.5 * N * (N * t).sum(-1, keepdims=True)
    w = np.where(rng.uniform(0., 1., n) < 0.5, -1., 1.) * np.where(rng.uniform(0., 1., n) < 0.8, 1., rng.uniform(0.2, 1., n))
    g[:, on:on + 3], g[:, ot:ot + 3], g[:, ot + 3] = nn, t, w
    d = np.concatenate([rng.uniform(-1., 1., (n, 2)), rng.uniform(MIN_Z + 0.01, 1., (n, 1))], 1)
    return g, ((d + 1.) / 2. if encoded else d).astype(np.float32)


def draw_pixels(rng, n, cg, on, ot, encoded=True, max_rejected=0.05):
    """Random pixels with every frame well conditioned (MIN_SIN, MIN_Z): draw, reject, redraw the rejected pixels; the share
    rejected from the first draw must stay under `max_rejected`.  -> (gbuffer, normal_map, share)"""
    g, m = random_pixels(rng, n, cg, on, ot, encoded)
    share = None
    for _ in range(20):
        r = perturb_gbuffer(g, m, on, ot, 1., encoded)
        bad = ~r['valid'] | (r['sin'] < MIN_SIN) | (r['z'] < MIN_Z)
        if share is None:
            share = float(bad.mean())
            assert share < max_rejected, 'share of rejected pixels %.3f' % share
        if not bad.any():
            return g, m, share
        g[bad], m[bad] = random_pixels(rng, int(bad.sum()), cg, on, ot, encoded)
    raise AssertionError('could not draw pixels with well-conditioned frames')


if __name__ == '__main__':
    from tests import test_normal_map
    meshes, pixels = test_normal_map.tolerance_cases()
    print({k: '%.3e' % v for k, v in measure_f32(meshes, pixels).items()})
