"""The restatement `dirt_amd.shading.shade_gbuffer` is checked against: no arithmetic of its own, it calls the functions of
dirt_amd/lighting.py (pinned to the reference's source by tests/test_helpers_ref.py) on CPU tensors, composes them as
DESIGN.md §7b says and takes gradients with torch's autograd.  Every parameter is expanded to one row per pixel and made a
leaf, which the lighting functions' leading batch dimensions allow: a parameter's gradient is the sum of its leaf's rows,
its L1 mass the sum of their absolute values.  Run in float64 it is the reference; run in float32 it is the
implementation users had before the kernel, whose error sets the tolerance (`measure_f32`).

    python -m tests.shade_reference      # prints the float32 figures the constants of tests/test_shade.py restate
"""
import numpy as np
import torch

from dirt_amd import lighting

SAMPLE_LAYOUT = dict(colors=4, normals=7, positions=1, mask=0)   # examples/deferred.py: mask, position, colour, normal


def _rows(x, width, dtype):
    """a parameter -> [R, width] tensor of `dtype` (R = 1: shared by the scenes)"""
    t = torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)).to(dtype)
    return t.reshape(-1, width)


class _SplitTorch:
    """`torch` as dirt_amd/lighting.py sees it while the MASS of d gbuffer is taken: the same values, but the two places where a
    gradient cancels inside one term are cut into separate autograd paths, so that their absolute values can be added.
    `vector_norm(x)` is taken of a detached copy of x that is a leaf: the half of d (x / |x|) / d x that flows through the norm
    arrives at that leaf, the other half at x.  `matmul(normals, light)` likewise: the (n . l) factor of the reflected
    direction 2 (n . l) n arrives at a leaf copy of the normals, the direct n at the normals.  Nothing else differs."""

    def __init__(self):
        self.norm_leaves, self.matmul_leaves, self.linalg = [], [], self

    def __getattr__(self, name):
        return getattr(torch, name)

    def vector_norm(self, x, **kw):
        leaf = x.detach().requires_grad_(True)
        self.norm_leaves.append(leaf)
        return torch.linalg.vector_norm(leaf, **kw)

    def matmul(self, a, b):
        leaf = a.detach().requires_grad_(True)
        self.matmul_leaves.append(leaf)
        return torch.matmul(leaf, b)


def compose(gbuffer, lights, layout, ambient=(0., 0., 0.), camera_position=None, background=(0., 0., 0.), clamp=(0., 1.),
            grad_out=None, scene_index=None, dtype=torch.float64, masses=True, _split=None):
    """gbuffer [N, Cg] (float32 values), lights as `shade_gbuffer` takes them, scene_index [N] (pixel -> scene) for per-scene
    parameters.  -> dict: out, pre (before the clamp), cosines [N, lights], mass_out; with grad_out [N, 3] also d_gbuffer,
    mass_gbuffer and d_params / mass_params {name: [R, width]} (names: 'ambient', 'background', 'camera_position',
    'light<i>.vector', 'light<i>.color', 'light<i>.shininess')."""
    g = torch.as_tensor(np.asarray(gbuffer, dtype=np.float32)).to(dtype).requires_grad_(True)
    n_px = g.shape[0]
    idx = torch.zeros(n_px, dtype=torch.long) if scene_index is None else torch.as_tensor(np.asarray(scene_index)).long()
    shared, leaves = {}, {}

    def leaf(name, x, width):
        shared[name] = _rows(x, width, dtype)
        r = shared[name]
        leaves[name] = r[idx if r.shape[0] > 1 else torch.zeros_like(idx)].clone().requires_grad_(True)
        return leaves[name]

    c = g[:, layout['colors']:layout['colors'] + 3]
    n = g[:, layout['normals']:layout['normals'] + 3]
    p = g[:, layout['positions']:layout['positions'] + 3] if layout.get('positions') is not None else None
    m = g[:, layout['mask']:layout['mask'] + 1] if layout.get('mask') is not None else torch.ones(n_px, 1, dtype=dtype)
    amb, bg = leaf('ambient', ambient, 3), leaf('background', background, 3)
    cam = leaf('camera_position', camera_position, 3) if camera_position is not None else None
    terms, cosines = [amb * c], []
    if _split is not None:
        lighting.torch = _split
    try:
        _light_terms(lights, leaf, n, c, p, cam, terms, cosines)
    finally:
        lighting.torch = torch
    return _finish(g, layout, terms, cosines, m, bg, clamp, grad_out, idx, shared, leaves, dtype, masses, _split,
                   dict(gbuffer=gbuffer, lights=lights, layout=layout, ambient=ambient, camera_position=camera_position, background=background,
                        clamp=clamp, grad_out=grad_out, scene_index=scene_index, dtype=dtype))


def _light_terms(lights, leaf, n, c, p, cam, terms, cosines):
    for i, rec in enumerate(lights):
        kind, ds = rec[0], bool(rec[-1])
        vec, col = leaf('light%d.vector' % i, rec[1], 3), leaf('light%d.color' % i, rec[2], 3)
        if kind == 'diffuse_directional':
            t = lighting.diffuse_directional(n[:, None], c[:, None], vec, col, double_sided=ds)
            cos = -(n * vec).sum(-1)
        elif kind == 'specular_directional':
            s = leaf('light%d.shininess' % i, rec[3], 1)
            t = lighting.specular_directional(p[:, None], n[:, None], c[:, None], vec, col, cam, s[:, 0], double_sided=ds)
            to_cam = cam - p
            refl = vec + 2. * (n * -vec).sum(-1, keepdim=True) * n
            cos = ((to_cam / to_cam.norm(dim=-1, keepdim=True) + 1.e-12) * refl).sum(-1)
        elif kind == 'diffuse_point':
            t = lighting.diffuse_point(p[:, None], n[:, None], c[:, None], vec, col, double_sided=ds)
            rel = p - vec
            cos = (n * rel / (rel.norm(dim=-1, keepdim=True) + 1.e-12)).sum(-1)
        else:
            raise ValueError(kind)
        terms.append(t[:, 0])
        cosines.append(cos.detach())   # for keeping test data off the kinks only; the check itself uses `t`


def _finish(g, layout, terms, cosines, m, bg, clamp, grad_out, idx, shared, leaves, dtype, masses, _split, again):
    n_px = g.shape[0]
    lit = terms[0]
    for t in terms[1:]:
        lit = lit + t
    pre = lit * m + bg * (1. - m)
    out = torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre
    parts = [t * m for t in terms] + [bg * (1. - m)]   # the terms that add up to a pixel
    res = {'out': out.detach(), 'pre': pre.detach(), 'cosines': torch.stack(cosines, 1) if cosines else torch.zeros(n_px, 0, dtype=dtype),
           'mass_out': sum(q.detach().abs() for q in parts)}
    if grad_out is None:
        return res
    if _split is not None:
        return _split_mass(g, layout, parts, pre, clamp, grad_out, dtype, _split)
    go = torch.as_tensor(np.asarray(grad_out, dtype=np.float32)).to(dtype)
    names = list(leaves)
    grads = torch.autograd.grad((out * go).sum(), [g] + [leaves[k] for k in names], retain_graph=True, allow_unused=True)
    zero = lambda like, x: torch.zeros_like(like) if x is None else x   # noqa: E731
    res['d_gbuffer'] = zero(g, grads[0])
    res['d_params'], res['mass_params'] = {}, {}
    for k, gr in zip(names, grads[1:]):
        gr = zero(leaves[k], gr)
        rows = shared[k].shape[0]
        at = idx if rows > 1 else torch.zeros_like(idx)
        res['d_params'][k] = torch.zeros(rows, gr.shape[1], dtype=dtype).index_add_(0, at, gr)
        res['mass_params'][k] = torch.zeros(rows, gr.shape[1], dtype=dtype).index_add_(0, at, gr.abs())
    if masses:
        res['mass_gbuffer'] = compose(masses=False, _split=_SplitTorch(), **again)
    return res


def _split_mass(g, layout, parts, pre, clamp, grad_out, dtype, split):
    """The L1 mass of d gbuffer: per term, per output channel and, inside a term, per autograd path where _SplitTorch cut one."""
    go = torch.as_tensor(np.asarray(grad_out, dtype=np.float32)).to(dtype)
    gate = ((pre >= clamp[0]) & (pre <= clamp[1])).to(dtype).detach() if clamp is not None else torch.ones_like(pre)
    mass = torch.zeros_like(g)
    extra = [(leaf, 'positions') for leaf in split.norm_leaves] + [(leaf, 'normals') for leaf in split.matmul_leaves]
    for q in parts:
        for ch in range(3):
            grads = torch.autograd.grad((gate[:, ch] * go[:, ch] * q[:, ch]).sum(), [g] + [leaf for leaf, _ in extra], retain_graph=True,
                                        allow_unused=True)
            if grads[0] is not None:
                mass += grads[0].abs()
            for (leaf, attr), gr in zip(extra, grads[1:]):
                if gr is not None:   # the leaf is [N, 1, 3]: camera - p, p - light (d / d p = -1, +1) or the normals themselves
                    mass[:, layout[attr]:layout[attr] + 3] += gr[:, 0].abs()
    return mass.detach()


def off_kinks(res, clamp, margin=1.e-3):
    """[N] bool: the pixel's cosines and pre-clamp values are at least `margin` from 0, lo and hi."""
    ok = (res['cosines'].abs() >= margin).all(1)
    if clamp is not None:
        ok &= ((res['pre'] - clamp[0]).abs() >= margin).all(1) & ((res['pre'] - clamp[1]).abs() >= margin).all(1)
    return ok


def sample_lights(light_direction, camera_position=None):
    """the lights, ambient and background of examples/deferred.py::shader_fn -> (lights, keyword arguments)"""
    lights = [('diffuse_directional', light_direction, (1., 0., 0.), False),
              ('specular_directional', light_direction, (1., 1., 1.), 6., False)]
    return lights, dict(ambient=(0.2, 0.2, 0.2), background=(0., 0., 0.3), clamp=(0., 1.), camera_position=camera_position)


def random_lights(rng, kinds, double_sided, batch=None):
    """`len(kinds)` lights with unit directions, positions a few units away, colours in [0.2, 1], shininess in [1, 32];
    batch: one value per scene ([batch, 3] / [batch])."""
    shape = (3,) if batch is None else (batch, 3)
    out = []
    for k, kind in enumerate(kinds):
        v = rng.standard_normal(shape).astype(np.float32)
        col = rng.uniform(0.2, 1., shape).astype(np.float32)
        ds = double_sided if isinstance(double_sided, bool) else bool(double_sided[k])
        if kind == 'diffuse_point':
            out.append((kind, (v * 3.).astype(np.float32), col, ds))
        else:
            v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
            if kind == 'specular_directional':
                out.append((kind, v, col, rng.uniform(1., 32., shape[:-1]).astype(np.float32), ds))
            else:
                out.append((kind, v, col, ds))
    return out


def random_gbuffer(rng, n, cg, layout, covered=0.7):
    """[n, cg] float32: uniform colours, unit normals, positions in [-1, 1]^3, a mask of 0 / 1 / fractional coverage; the
    channels no attribute uses hold noise (the kernel must ignore them)."""
    g = rng.standard_normal((n, cg)).astype(np.float32)
    g[:, layout['colors']:layout['colors'] + 3] = rng.uniform(0.05, 1., (n, 3))
    nn = rng.standard_normal((n, 3))
    g[:, layout['normals']:layout['normals'] + 3] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    if layout.get('positions') is not None:
        g[:, layout['positions']:layout['positions'] + 3] = rng.uniform(-1., 1., (n, 3))
    if layout.get('mask') is not None:
        u = rng.uniform(0., 1., n)
        g[:, layout['mask']] = np.where(u < covered, 1., np.where(u < covered + 0.1, rng.uniform(0.1, 0.9, n), 0.))
    return g


def draw_off_kinks(rng, n, cg, layout, lights, kw, scene_index=None, max_rejected=0.05, covered=0.7):
    """A random G-buffer whose pixels all stay off the kinks: draw, reject against the float64 restatement, redraw the rejected
    pixels.  The share rejected from the first draw must stay under `max_rejected`.  -> (gbuffer, share)"""
    g = random_gbuffer(rng, n, cg, layout, covered)
    share = None
    for _ in range(20):
        bad = ~off_kinks(compose(g, lights, layout, scene_index=scene_index, **kw), kw.get('clamp', (0., 1.))).numpy()
        if share is None:
            share = bad.mean()
            assert share < max_rejected, 'share of rejected pixels %.3f' % share
        if not bad.any():
            return g, share
        g[bad] = random_gbuffer(rng, int(bad.sum()), cg, layout, covered)
    raise AssertionError('could not draw pixels off the kinks')


# float32 cannot hold what float64 can: pow(0.005, 30) is 1e-69.  An intermediate that underflows (below 2^-126) is lost whole,
# and the factors applied after it (colours, shininess, 1 / distance: 2^26 is generous) scale the loss.  Errors below this floor
# are the number format's, in the float32 composition as in the kernel, and are not counted against the mass.
UNDERFLOW_FLOOR = 2. ** -100


def attribute_slices(layout):
    """{attribute: slice of its channels} for the attributes the layout has"""
    return {k: slice(layout[k], layout[k] + (1 if k == 'mask' else 3)) for k in ('colors', 'normals', 'positions', 'mask') if layout.get(k) is not None}


def worst_ratio(got, ref, mass):
    """max (|got - ref| - UNDERFLOW_FLOOR) / mass over the elements with mass > 0 (0 if there are none)"""
    got, ref, mass = (np.asarray(x, dtype=np.float64) for x in (got, ref, mass))
    pos = mass > 0
    return float((np.maximum(np.abs(got - ref)[pos] - UNDERFLOW_FLOOR, 0.) / mass[pos]).max()) if pos.any() else 0.


def measure_f32(cases):
    """cases: iterable of (gbuffer, lights, layout, kw, grad_out, scene_index) -> the worst |f32 - f64| / mass of the float32
    composition per kind of result: {'pixels', 'd_colors', 'd_normals', 'd_positions', 'd_mask', 'd_params'} (d gbuffer by
    attribute)."""
    worst = {'pixels': 0., 'd_colors': 0., 'd_normals': 0., 'd_positions': 0., 'd_mask': 0., 'd_params': 0.}
    for g, lights, layout, kw, go, idx in cases:
        r64 = compose(g, lights, layout, grad_out=go, scene_index=idx, dtype=torch.float64, **kw)
        r32 = compose(g, lights, layout, grad_out=go, scene_index=idx, dtype=torch.float32, masses=False, **kw)
        worst['pixels'] = max(worst['pixels'], worst_ratio(r32['out'], r64['out'], r64['mass_out']))
        for name, sl in attribute_slices(layout).items():
            worst['d_' + name] = max(worst['d_' + name], worst_ratio(r32['d_gbuffer'][:, sl], r64['d_gbuffer'][:, sl], r64['mass_gbuffer'][:, sl]))
        for k in r64['d_params']:
            worst['d_params'] = max(worst['d_params'], worst_ratio(r32['d_params'][k], r64['d_params'][k], r64['mass_params'][k]))
    return worst


if __name__ == '__main__':
    from tests import test_shade
    print(measure_f32(test_shade.tolerance_cases()))
