"""The restatement `dirt_amd.geometry.vertex_stage` is checked against: it calls `vertex_normals` / `vertex_normals_pre_split`
of dirt_amd/lighting.py (pinned to the reference's source by tests/test_helpers_ref.py) and two matmuls on CPU tensors,
composes them as DESIGN.md §7c says and takes gradients with torch's autograd.  Run in float64 it is the reference; run
in float32 it is the implementation users had before the kernel, whose error sets the tolerance (`measure_f32`).

Beside every result it returns, per element, the L1 mass of the terms summed into that element: the scale an error of
that element is measured against.  Values and gradients come from lighting.py and autograd alone; only the masses are
written out here, in float64, as the same sums with every term replaced by its absolute value:

    world    |v4| @ |model|                          clip    (|v4| @ |model|) @ |view_projection|
    n = e1 x e2                                      m(n)  = |e1| (x) |e2|   (both products of each component, added)
    fn = n / (|n| + 1e-12)                           m(fn) = m(n) / (|n| + 1e-12) + |n| (|n| . m(n)) / (|n| (|n| + 1e-12)^2)
    s = sum of fn                                    m(s)  = sum of m(fn);   normals: the same rule as fn, from s and m(s)
    backwards the same way: d s from d normals, d fn = sum of three d s, d n from d fn, d e1 = e2 x d n, d e2 = d n x e1,
    the corners' sums, + |d world| + |d clip| @ |view_projection|^T, through |model|^T to d vertices;
    d model = sum of |v4|^T m(d world4), d view_projection = sum of m(world4)^T |d clip|.
The edges e = w1 - w0 are taken as they are (their cancellation is bounded by the meshes, see `grid_mesh`).

    python -m tests.geometry_reference      # prints the float32 figures the constants of tests/test_geometry.py restate
"""
import numpy as np
import torch

from dirt_amd import lighting

EPS = 1.e-12

# What the generators of the non-degenerate meshes guarantee for every face, in object space: its area is at least
# MIN_AREA_RATIO x (longest edge)^2 and its smallest angle at least MIN_ANGLE_DEG.  A right triangle with equal legs has
# ratio 0.25 and 45 degrees; the jitter below keeps the grid's triangles within about a factor 2 of that.  With these the
# float32 cross product keeps 2^-24 / sin(15 deg) ~ 2.3e-7 relative accuracy per face: the composition stays finite and
# well-conditioned (tests/test_geometry.py::test_meshes_keep_their_bounds checks both, on the CPU).
MIN_AREA_RATIO = 0.06
MIN_ANGLE_DEG = 15.


# ------------------------------------------------------------------------------------------------------------ meshes

def grid_mesh(rng, num_vertices, jitter=0.2):
    """A shared-vertex mesh of exactly `num_vertices` vertices: the first vertices, row by row, of a square grid over
    [-1, 1]^2 with the two triangles of every complete cell; x, y jittered by `jitter` cells and z by 1.5 x that.
    -> (vertices [V, 3] float32, faces [F, 3] int32); F is about 2 V (0 for V < 3)."""
    cols = max(2, int(np.ceil(np.sqrt(num_vertices))))
    h = 2. / cols
    idx = np.arange(num_vertices)
    xy = np.stack([idx % cols, idx // cols], 1) * h - 1.
    v = np.concatenate([xy + rng.uniform(-jitter, jitter, (num_vertices, 2)) * h,
                        rng.uniform(-1.5 * jitter, 1.5 * jitter, (num_vertices, 1)) * h], 1).astype(np.float32)
    a = idx[(idx % cols < cols - 1) & (idx + cols + 1 < num_vertices)]
    faces = np.concatenate([np.stack([a, a + 1, a + cols + 1], 1), np.stack([a, a + cols + 1, a + cols], 1)]).astype(np.int32)
    lone = idx[(idx % cols < cols - 1) & (idx + cols < num_vertices) & (idx + cols + 1 >= num_vertices)]   # the last, incomplete cell: one triangle
    faces = np.concatenate([faces, np.stack([lone, lone + 1, lone + cols], 1).astype(np.int32)])
    return v, faces.reshape(-1, 3)


def fan_mesh(rng, blades=2000):
    """One vertex in `blades` faces: a pinwheel of well-shaped triangles that share vertex 0 and nothing else (they overlap
    in space, which the vertex stage does not mind), all wound the same way so that the hub's normal is a long sum.
    -> (vertices [1 + 2 blades, 3], faces [blades, 3])"""
    v = np.concatenate([np.zeros((1, 3)), _pinwheel_rim(rng, blades).reshape(-1, 3)]).astype(np.float32)
    b = np.arange(blades)
    return v, np.stack([np.zeros_like(b), 1 + 2 * b, 2 + 2 * b], 1).astype(np.int32)


def _pinwheel_rim(rng, blades):
    """The two rim vertices of every blade of a pinwheel around the origin: an opening of 40 to 80 degrees between two
    edges of length 0.6 to 1, a little out of the plane.  -> [blades, 2, 3] float64"""
    theta = rng.uniform(0., 2. * np.pi, blades)
    open_ = np.deg2rad(rng.uniform(40., 80., blades))
    r = rng.uniform(0.6, 1., (blades, 2))
    rim = np.zeros((blades, 2, 3))
    for k, ang in enumerate((theta, theta + open_)):
        rim[:, k, 0], rim[:, k, 1] = r[:, k] * np.cos(ang), r[:, k] * np.sin(ang)
        rim[:, k, 2] = rng.uniform(-0.1, 0.1, blades)
    return rim


def hubs_mesh(rng, hubs):
    """Several fans in one mesh.  hubs: [(vertex index, blades)]; every hub is the centre, somewhere in [-0.5, 0.5]^3, of a
    pinwheel like `fan_mesh`'s with two private rim vertices per blade; the rim vertices take the indices the hubs leave,
    in order (hub after hub, blade after blade).  The faces are ordered by hub, then blade: (hub, rim, rim), so a hub's
    list has `blades` entries and a rim vertex's one.
    -> (vertices [len(hubs) + 2 sum(blades), 3], faces [sum(blades), 3])"""
    total = len(hubs) + 2 * sum(blades for _, blades in hubs)
    at = [h for h, _ in hubs]
    assert len(set(at)) == len(at) and all(0 <= h < total for h in at), (at, total)
    free = np.setdiff1d(np.arange(total), at)
    v, faces, used = np.zeros((total, 3)), [], 0
    for h, blades in hubs:
        centre = rng.uniform(-0.5, 0.5, 3)
        slots = free[used:used + 2 * blades]
        used += 2 * blades
        v[h], v[slots] = centre, (_pinwheel_rim(rng, blades) + centre).reshape(-1, 3)
        faces.append(np.stack([np.full(blades, h), slots[0::2], slots[1::2]], 1))
    return v.astype(np.float32), np.concatenate(faces).astype(np.int32)


def split_mesh(vertices, faces):
    """`lighting.split_vertices_by_face` in numpy: every vertex used by exactly one face"""
    return np.ascontiguousarray(vertices[..., faces.reshape(-1), :]), np.arange(faces.size, dtype=np.int32).reshape(-1, 3)


def face_quality(vertices, faces):
    """-> (smallest area / longest edge^2, smallest angle in degrees) over the faces of [V, 3|4] vertices"""
    if not len(faces):
        return np.inf, 180.
    p = np.asarray(vertices, np.float64)[..., :3][faces]               # [F, 3, 3]
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], 1)
    ln = np.linalg.norm(e, axis=-1)
    area = 0.5 * np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=-1)
    cosines = [-(e[:, k] * e[:, (k + 2) % 3]).sum(-1) / (ln[:, k] * ln[:, (k + 2) % 3]) for k in range(3)]
    return float((area / ln.max(1) ** 2).min()), float(np.rad2deg(np.arccos(np.clip(np.max(cosines, 0), -1., 1.))).min())


def random_model(rng, batch=None):
    """rotation x scale in [0.6, 1.4] + translation (row-vector convention: the last ROW translates), and a last column a
    little off (0, 0, 0, 1) so that w is not trivially 1.  -> [4, 4] or [batch, 4, 4] float32"""
    out = []
    for _ in range(batch or 1):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        m = np.eye(4)
        m[:3, :3] = q * rng.uniform(0.6, 1.4)
        m[3, :3] = rng.uniform(-0.5, 0.5, 3)
        m[:, 3] += rng.uniform(-0.02, 0.02, 4)
        out.append(m)
    return np.asarray(out if batch else out[0], np.float32)


def random_view_projection(rng, batch=None):
    """a view (rotation, 3 units back) times the perspective projection of the samples -> [4, 4] or [batch, 4, 4] float32"""
    from dirt_amd import matrices
    out = []
    for _ in range(batch or 1):
        view = matrices.compose(matrices.rodrigues(torch.from_numpy(rng.uniform(-0.4, 0.4, 3).astype(np.float32))),
                                matrices.translation(torch.tensor([0., 0., -3.]) + torch.from_numpy(rng.uniform(-0.2, 0.2, 3).astype(np.float32))))
        out.append((view @ matrices.perspective_projection(near=0.1, far=20., right=0.1, aspect=0.75)).numpy())
    return np.asarray(out if batch else out[0], np.float32)


# ------------------------------------------------------------------------------------------------------------ the restatement

def _t(x, dtype):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)


def _abs_cross(a, b):
    """|a| (x) |b|: the two products of every component of a cross product, added"""
    a, b = a.abs(), b.abs()
    return torch.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _mass_of_normalised(x, mass_x):
    """y = x / (|x| + 1e-12): the direct term and the one through the norm (absent at x = 0, as its gradient is)"""
    ln = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    through = torch.where(ln > 0, x.abs() * (x.abs() * mass_x).sum(-1, keepdim=True) / (ln.clamp_min(1e-300) * (ln + EPS) ** 2), torch.zeros_like(x))
    return mass_x / (ln + EPS) + through


def _scatter(values, faces, num_vertices):
    """values [B, F, 3 corners, 3] -> [B, V, 3]: every corner's row added to its vertex"""
    out = torch.zeros(values.shape[0], num_vertices, 3, dtype=values.dtype)
    for k in range(3):
        out = out.index_add(1, faces[:, k], values[:, :, k])
    return out


def compose(vertices, faces, model=None, view_projection=None, pre_split=False, grads=None, dtype=torch.float64, masses=True):
    """vertices [V, 3|4] or [B, V, 3|4], faces [F, 3], model / view_projection [4, 4], [B, 4, 4] or None (float32 values);
    grads: {'clip' / 'world' / 'normals': d loss / d output, or absent}.
    -> dict of float tensors: clip (None without a view_projection), world, normals; with `grads` also d_vertices, d_model,
    d_view_projection (None where there is no such input); with `masses` a 'mass_' + name beside each (float64 only)."""
    vertices = np.asarray(vertices, np.float32)
    batched = vertices.ndim == 3
    v = _t(vertices if batched else vertices[None], dtype).requires_grad_(True)
    f = torch.as_tensor(np.asarray(faces)).long().reshape(-1, 3)
    B, V, C = v.shape
    v4 = v if C == 4 else torch.cat([v, torch.ones_like(v[..., :1])], -1)
    M = _t(model, dtype).reshape(-1, 4, 4).requires_grad_(True) if model is not None else None
    P = _t(view_projection, dtype).reshape(-1, 4, 4).requires_grad_(True) if view_projection is not None else None
    world = v4 @ M if M is not None else v4
    clip = world @ P if P is not None else None
    normals = (lighting.vertex_normals_pre_split if pre_split else lighting.vertex_normals)(world, f)
    unb = (lambda x: x if batched or x is None else x[0])
    res = {'clip': unb(clip.detach()) if clip is not None else None, 'world': unb(world.detach()), 'normals': unb(normals.detach())}
    if masses:
        assert dtype == torch.float64
        with torch.no_grad():
            m_world = v4.abs() @ M.abs() if M is not None else v4.abs()
            w = world[..., :3]
            w0, w1, w2 = (w[:, f[:, k]] for k in range(3))
            e1, e2 = w1 - w0, w2 - w0
            n = torch.linalg.cross(e1, e2, dim=-1)
            ln = torch.linalg.vector_norm(n, dim=-1, keepdim=True)
            m_fn = _mass_of_normalised(n, _abs_cross(e1, e2))
            fn = n / (ln + EPS)
            s = _scatter(fn[:, :, None].expand(-1, -1, 3, -1), f, V)
            m_s = _scatter(m_fn[:, :, None].expand(-1, -1, 3, -1), f, V)
            res['mass_world'] = unb(m_world)
            res['mass_clip'] = unb(m_world @ P.abs()) if P is not None else None
            res['mass_normals'] = unb(m_s if pre_split else _mass_of_normalised(s, m_s))
    if grads is None:
        return res
    g = {k: (_t(grads[k], dtype).reshape(x.shape) if grads.get(k) is not None and x is not None else None)
         for k, x in (('clip', clip), ('world', world), ('normals', normals))}
    loss = sum((x * g[k]).sum() for k, x in (('clip', clip), ('world', world), ('normals', normals)) if g[k] is not None)
    leaves = [t for t in (v, M, P) if t is not None]
    got = iter(torch.autograd.grad(loss, leaves, allow_unused=True)) if isinstance(loss, torch.Tensor) and loss.requires_grad else iter([None] * 3)
    for name, leaf, shape in (('d_vertices', v, vertices.shape), ('d_model', M, np.shape(model)), ('d_view_projection', P, np.shape(view_projection))):
        if leaf is None:
            res[name] = None
            continue
        gr = next(got)
        res[name] = (torch.zeros_like(leaf) if gr is None else gr).reshape(shape)
    if not masses:
        return res
    with torch.no_grad():
        zero3 = torch.zeros(B, V, 3, dtype=dtype)
        if g['normals'] is None:
            m_w3 = zero3
        else:
            gN = g['normals'].abs()
            if pre_split:
                m_gs = gN
            else:
                L = torch.linalg.vector_norm(s, dim=-1, keepdim=True)
                m_gs = gN / (L + EPS) + torch.where(L > 0, s.abs() * (gN * s.abs()).sum(-1, keepdim=True) / (L.clamp_min(1e-300) * (L + EPS) ** 2), zero3)
            m_gf = m_gs[:, f[:, 0]] + m_gs[:, f[:, 1]] + m_gs[:, f[:, 2]]
            m_gn = m_gf / (ln + EPS) + torch.where(ln > 0, n.abs() * (m_gf * n.abs()).sum(-1, keepdim=True) / (ln.clamp_min(1e-300) * (ln + EPS) ** 2),
                                                   torch.zeros_like(n))
            m_ge1, m_ge2 = _abs_cross(e2, m_gn), _abs_cross(m_gn, e1)
            m_w3 = _scatter(torch.stack([m_ge1 + m_ge2, m_ge1, m_ge2], 2), f, V)
        m_G = torch.zeros(B, V, 4, dtype=dtype)
        m_G[..., :3] += m_w3
        if g['world'] is not None:
            m_G += g['world'].abs()
        if g['clip'] is not None:
            m_G += g['clip'].abs() @ P.abs().transpose(-1, -2)
        m_dv = (m_G @ M.abs().transpose(-1, -2) if M is not None else m_G)[..., :C]
        res['mass_d_vertices'] = m_dv.reshape(vertices.shape)
        per_scene = lambda x, like: x if like.shape[0] > 1 else x.sum(0, keepdim=True)   # noqa: E731
        res['mass_d_model'] = per_scene(v4.abs().transpose(-1, -2) @ m_G, M).reshape(np.shape(model)) if M is not None else None
        m_gc = g['clip'].abs() if g['clip'] is not None else torch.zeros(B, V, 4, dtype=dtype)
        res['mass_d_view_projection'] = per_scene(m_world.transpose(-1, -2) @ m_gc, P).reshape(np.shape(view_projection)) if P is not None else None
    return res


VALUE_KINDS = ('clip', 'world', 'normals')
GRAD_KINDS = ('d_vertices', 'd_model', 'd_view_projection')


def worst_ratio(got, ref, mass):
    """max |got - ref| / mass over the elements with mass > 0 (0 if there are none)"""
    got, ref, mass = (np.asarray(x, dtype=np.float64) for x in (got, ref, mass))
    pos = (mass > 0) & np.isfinite(mass) & np.isfinite(ref)
    return float((np.abs(got - ref)[pos] / mass[pos]).max()) if pos.any() else 0.


def measure_f32(cases):
    """cases: iterable of keyword dicts for `compose` -> the worst |f32 - f64| / mass of the float32 composition per kind of
    result: {'clip', 'world', 'normals', 'd_vertices', 'd_model', 'd_view_projection'}"""
    worst = {k: 0. for k in VALUE_KINDS + GRAD_KINDS}
    for kw in cases:
        r64 = compose(dtype=torch.float64, **kw)
        r32 = compose(dtype=torch.float32, masses=False, **kw)
        for k in worst:
            if r64.get(k) is not None:
                worst[k] = max(worst[k], worst_ratio(r32[k], r64[k], r64['mass_' + k]))
    return worst


if __name__ == '__main__':
    from tests import test_geometry
    for name, value in measure_f32(test_geometry.tolerance_cases()).items():
        print('%-20s %.3e' % (name, value))
