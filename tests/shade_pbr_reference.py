"""The restatement `dirt_amd.shading.shade_gbuffer_pbr` is checked against: `dirt_amd.lighting.cook_torrance` on CPU tensors,
the ambient term, the mask composite and the clamp of DESIGN.md §7b, gradients by torch's autograd.  Every parameter is
expanded to one row per pixel and made a leaf: a parameter's gradient is the sum of its leaf's rows.  Run in float64 it is
the reference; run in float32 it is the composition users had before the kernel, whose error sets the tolerance
(`measure_f32`).

The L1 mass of an element is taken per term (ambient, each light's diffuse and specular lobe, background), per output channel
and, inside a term, per autograd path where a gradient cancels (`_SplitTorch`):
  - at every normalisation x / max(|x|, 1e-12) the norm is taken of a detached leaf copy of x, so the half of the gradient that
    flows through the norm and the direct half -- which cancel along x -- are added by their absolute values;
  - a2 enters den = |n x h|^2 + a2 nh^2 through a leaf copy (`torch.mul` in lighting.py), which parts D's numerator from its
    denominator: d D / d a2 = (|n x h|^2 - a2 nh^2) / (pi den^3) cancels where tan^2(theta) = a2;
  - a lobe's term is cut into the three products of n^ . l, which cancel where a light grazes the surface (`fine` in `compose`).
What arrives at a leaf copy is carried on to the inputs by a backward pass of its own (`_path_masses`), which meets the inner
cuts' leaves in turn.  Per term only, the float32 composition's d material read 1.1e-5 to 1.5e-5; with the cuts every kind
reads below 3e-6.

    python -m tests.shade_pbr_reference      # prints the float32 figures the constants of tests/test_shade_pbr.py restate
"""
import numpy as np
import torch

from dirt_amd import lighting
from tests.shade_reference import worst_ratio

ATTRIBUTES = (('colors', 3), ('material', 2), ('normals', 3), ('positions', 3), ('mask', 1))
KINDS = ('pixels', 'd_colors', 'd_material', 'd_normals', 'd_positions', 'd_mask', 'd_params')


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)).to(dtype)


class _SplitTorch:
    """`torch` as dirt_amd/lighting.py sees it while the masses are taken: the same values, but `normalize(x)` divides x by the
    norm of a detached leaf copy of x, and `mul(a, b)` multiplies a detached leaf copy of a.  `cuts` lists (leaf, original)."""

    def __init__(self):
        self.cuts, self.nn, self.functional, self.linalg = [], self, self, self

    def __getattr__(self, name):
        return getattr(torch, name)

    def normalize(self, x, dim=-1, eps=1.e-12):
        leaf = x.detach().requires_grad_(True)
        self.cuts.append((leaf, x))
        return x / torch.linalg.vector_norm(leaf, dim=dim, keepdim=True).clamp_min(eps)

    def cross(self, a, b, dim=-1):
        return torch.linalg.cross(a, b, dim=dim)

    def mul(self, a, b):
        leaf = a.detach().requires_grad_(True)
        self.cuts.append((leaf, a))
        return torch.mul(leaf, b)


def param_names(n_lights):
    return ['ambient', 'background', 'camera_position'] + [k % i for i in range(n_lights) for k in ('light%d.vector', 'light%d.color')]


def compose(gbuffer, lights, layout, colors=None, material=None, ambient=(0., 0., 0.), camera_position=(0., 0., 4.),
            background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04, grad_out=None, scene_index=None,
            dtype=torch.float64, masses=True, drop=None, swap_material=False):
    """gbuffer [N, Cg] (float32 values); lights as `shade_gbuffer_pbr` takes them, vectors and colours [3] or [R, 3], like
    ambient, camera_position and background, with scene_index [N] (pixel -> row); layout: first channels of colors, material,
    normals, positions, mask (colors / material absent with `colors` [N, 3] / `material` [N, 2] given; mask may be None).
    drop: (light, 'diffuse' or 'specular'): that lobe is left out; swap_material: roughness and metalness change places
    (both for the sensitivity checks).
    -> dict: out, pre, cosines [N, 1 + 3 lights] (n.v, then n.l, n.h, v.h per light, before the max), roughness; with grad_out
    [N, 3] also d_gbuffer, d_<attribute> ([N, 0] for an absent mask), d_params {name: [R, 3]}; with masses also mass_out and
    mass_<each of those>."""
    g = _t(gbuffer, dtype).requires_grad_(True)
    n_px = g.shape[0]
    idx = torch.zeros(n_px, dtype=torch.long) if scene_index is None else torch.as_tensor(np.asarray(scene_index)).long()
    col = _t(colors, dtype).requires_grad_(True) if colors is not None else None
    mat = _t(material, dtype).requires_grad_(True) if material is not None else None
    names = param_names(len(lights))
    values = [ambient, background, camera_position] + [x for rec in lights for x in rec[1:3]]
    shared = {k: _t(v, dtype).reshape(-1, 3) for k, v in zip(names, values)}
    at = lambda r: idx if r.shape[0] > 1 else torch.zeros_like(idx)   # noqa: E731
    leaves = {k: r[at(r)].clone().requires_grad_(True) for k, r in shared.items()}
    kinds = [rec[0] for rec in lights]
    has_mask = layout.get('mask') is not None

    def parts(gb, cl, mt):
        sl = lambda k, w: gb[:, layout[k]:layout[k] + w]   # noqa: E731
        c = cl if cl is not None else sl('colors', 3)
        rm = mt if mt is not None else sl('material', 2)
        m = sl('mask', 1) if has_mask else torch.ones(n_px, 1, dtype=dtype)
        r, mu = (rm[:, 1], rm[:, 0]) if swap_material else (rm[:, 0], rm[:, 1])
        return c, r, mu, sl('normals', 3), sl('positions', 3), m

    def terms(gb, cl, mt, lv, fine=False):
        """the terms that add up to a pixel before the clamp, in the order of the sum; fine: a lobe's term is cut once more,
        into the three products of n^ . l (which cancel where the light grazes the surface)"""
        c, r, mu, n, p, m = parts(gb, cl, mt)
        recs = [(kinds[i], lv['light%d.vector' % i], lv['light%d.color' % i]) for i in range(len(kinds))]
        lobes = lighting.cook_torrance_lobes(p[:, None], n[:, None], c[:, None], r[:, None], mu[:, None], lv['camera_position'], recs,
                                             min_roughness, dielectric_f0)
        out = [(lv['ambient'] * c) * m]
        for i, (diffuse, specular, weight, products) in enumerate(lobes):
            for name, lobe in (('diffuse', diffuse), ('specular', specular)):
                if drop == (i, name):
                    continue
                if fine:
                    lit = (products.sum(-1, keepdim=True) >= 0.).to(products.dtype)
                    out += [(lobe * (recs[i][2][:, None] * (products[..., j:j + 1] * lit)))[:, 0] * m for j in range(3)]
                else:
                    out.append((lobe * weight)[:, 0] * m)
        out.append(lv['background'] * (1. - m))
        return out, (c, r, mu, n, p, m, recs)

    # ---- values and gradients: lighting.cook_torrance itself
    _, (c, r, mu, n, p, m, recs) = terms(g, col, mat, leaves)
    if drop is None:
        lit = leaves['ambient'] * c + lighting.cook_torrance(p[:, None], n[:, None], c[:, None], r[:, None], mu[:, None], leaves['camera_position'],
                                                             recs, min_roughness, dielectric_f0)[:, 0]
        pre = lit * m + leaves['background'] * (1. - m)
    else:
        pre = sum(terms(g, col, mat, leaves)[0])
    out = torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre
    res = {'out': out.detach(), 'pre': pre.detach(), 'roughness': r.detach(), 'cosines': _cosines(n, p, leaves, kinds).detach()}

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
    if grad_out is not None:
        go = _t(grad_out, dtype)
        inputs = [g] + [leaves[k] for k in names] + [x for x in (col, mat) if x is not None]
        grads = [zero(x, gr) for x, gr in zip(inputs, torch.autograd.grad((out * go).sum(), inputs, allow_unused=True))]
        extra = grads[1 + len(names):]
        res.update(split(grads[0], extra[0] if col is not None else None, extra[-1] if mat is not None else None, 'd_'))
        res['d_params'] = {k: torch.zeros_like(shared[k]).index_add_(0, at(shared[k]), gr) for k, gr in zip(names, grads[1:])}
    if not masses:
        return res

    # ---- L1 masses: every term, output channel and autograd path apart
    gm = g.detach().clone().requires_grad_(True)
    cm = col.detach().clone().requires_grad_(True) if col is not None else None
    mm = mat.detach().clone().requires_grad_(True) if mat is not None else None
    lm = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    shim = _SplitTorch()
    lighting.torch = shim
    try:
        qs, _ = terms(gm, cm, mm, lm, fine=True)
    finally:
        lighting.torch = torch
    res['mass_out'] = sum(q.detach().abs() for q in qs)
    if grad_out is None:
        return res
    gate = ((pre >= clamp[0]) & (pre <= clamp[1])).to(dtype).detach() if clamp is not None else torch.ones_like(pre).detach()
    inputs = [gm] + [lm[k] for k in names] + [x for x in (cm, mm) if x is not None]
    mass = [torch.zeros_like(x) for x in inputs]
    for q in qs:
        if not q.requires_grad:
            continue
        for j in range(3):
            _path_masses((gate[:, j] * go[:, j] * q[:, j]).sum(), None, inputs, shim.cuts, mass)
    extra = mass[1 + len(names):]
    res.update(split(mass[0], extra[0] if cm is not None else None, extra[-1] if mm is not None else None, 'mass_'))
    res['mass_params'] = {k: torch.zeros_like(shared[k]).index_add_(0, at(shared[k]), ms) for k, ms in zip(names, mass[1:])}
    return res


def _path_masses(y, grad_y, inputs, cuts, mass):
    """adds to `mass` the absolute gradients of y (seeded with grad_y) at `inputs`, path by path: what arrives at the leaf of a
    cut is sent on through the tensor it was copied from"""
    work = [(y, grad_y)]
    while work:
        y, gy = work.pop()
        grads = torch.autograd.grad(y, inputs + [leaf for leaf, _ in cuts], grad_outputs=gy, retain_graph=True, allow_unused=True)
        for ms, gr in zip(mass, grads):
            if gr is not None:
                ms += gr.abs()
        for (leaf, origin), gr in zip(cuts, grads[len(inputs):]):
            if gr is not None and origin.requires_grad and bool(gr.any()):
                work.append((origin, gr))


def _cosines(n, p, lv, kinds):
    nrm = lambda x: torch.nn.functional.normalize(x, dim=-1, eps=1.e-12)   # noqa: E731
    N, v = nrm(n), nrm(lv['camera_position'] - p)
    cols = [(N * v).sum(-1)]
    for i, kind in enumerate(kinds):
        d = lv['light%d.vector' % i]
        l = nrm(d - p) if kind == 'point' else nrm(-d)
        h = nrm(l + v)
        cols += [(N * l).sum(-1), (N * h).sum(-1), (v * h).sum(-1)]
    return torch.stack(cols, 1)


def off_kinks(res, clamp, min_roughness=0.04, margin=1.e-3):
    """[N] bool: the pixel's cosines, its roughness and its pre-clamp values are at least `margin` from their kinks."""
    ok = (res['cosines'].abs() >= margin).all(1)
    ok &= ((res['roughness'] - min_roughness).abs() >= margin) & ((res['roughness'] - 1.).abs() >= margin)
    if clamp is not None:
        ok &= ((res['pre'] - clamp[0]).abs() >= margin).all(1) & ((res['pre'] - clamp[1]).abs() >= margin).all(1)
    return ok


def random_lights(rng, kinds, batch=None):
    """unit directions, positions a few units away, colours in [0.2, 0.6]; batch: one value per scene ([batch, 3]).
    The draw is tightened in one respect: seen from the origin, the direction towards a light has z > -0.5 (the camera sits
    near +z), others are redrawn.  A light shining at the camera from behind the scene makes l + v nearly cancel for every
    pixel of the frame: |l + v| loses its digits in float32, in the composition as in the kernel, and v . h sits at its kink
    for whole frames (a first draw then rejects a fifth of its pixels)."""
    shape = (3,) if batch is None else (batch, 3)
    out = []
    for kind in kinds:
        v = rng.standard_normal(shape)
        towards = (v if kind == 'point' else -v) / np.linalg.norm(v, axis=-1, keepdims=True)
        while (towards[..., 2] <= -0.5).any():
            v = rng.standard_normal(shape)
            towards = (v if kind == 'point' else -v) / np.linalg.norm(v, axis=-1, keepdims=True)
        v = v * 3. if kind == 'point' else v / np.linalg.norm(v, axis=-1, keepdims=True)
        out.append((kind, v.astype(np.float32), rng.uniform(0.2, 0.6, shape).astype(np.float32)))
    return out


def random_pixels(rng, n, cg, layout, covered=0.7):
    """(gbuffer [n, cg], colors [n, 3] or None, material [n, 2] or None): albedo U(0.05, 0.95), unit normals scaled by
    U(0.8, 1.2), positions in [-1, 1]^3, roughness U(0.25, 1), metalness U(0, 1), a mask of 0 / 1 / fractional coverage (70 % /
    10 % fractional); the channels no attribute uses hold noise."""
    g = rng.standard_normal((n, cg)).astype(np.float32)
    col = rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)
    mat = np.stack([rng.uniform(0.25, 1., n), rng.uniform(0., 1., n)], 1).astype(np.float32)
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


def draw_off_kinks(rng, n, cg, layout, lights, kw, scene_index=None, max_rejected=0.05):
    """Random pixels that all stay off the kinks: draw, reject against the float64 restatement, redraw the rejected pixels.
    The share rejected from the first draw must stay under `max_rejected`.  -> (gbuffer, colors or None, material or None, share)"""
    g, col, mat = random_pixels(rng, n, cg, layout)
    share = None
    for _ in range(20):
        ref = compose(g, lights, layout, colors=col, material=mat, scene_index=scene_index, masses=False, **kw)
        bad = ~off_kinks(ref, kw.get('clamp', (0., 1.)), kw.get('min_roughness', 0.04)).numpy()
        if share is None:
            share = float(bad.mean())
            assert share < max_rejected, 'share of rejected pixels %.3f' % share
        if not bad.any():
            return g, col, mat, share
        g[bad], c2, m2 = random_pixels(rng, int(bad.sum()), cg, layout)
        if col is not None:
            col[bad] = c2
        if mat is not None:
            mat[bad] = m2
    raise AssertionError('could not draw pixels off the kinks')


PAIRS = (('pixels', 'out', 'mass_out'),) + tuple(('d_' + k, 'd_' + k, 'mass_' + k) for k, _ in ATTRIBUTES)


def ratios(got, ref):
    """The worst |got - ref| / mass per kind of result; got: dict with out, d_<attribute>, d_params {name: tensor} (entries
    that are missing or None are skipped), ref: `compose(..., masses=True)`."""
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
    from tests import test_shade_pbr
    print({k: '%.3e' % v for k, v in measure_f32(c.measure() for c in test_shade_pbr.tolerance_cases().values()).items()})
