"""The restatement `dirt_amd.shading.shade_gbuffer_pbr(..., visibility=)` is checked against: `tests/shade_pbr_reference.compose`,
which already expands every parameter to one leaf row per pixel, with light i's row at a pixel holding `k_i * s_i` -- the
light's colour times the pixel's visibility.  The lighting function is linear in that row, so

    d s_i   = (the row's colour gradient) . k_i              mass:  (the row's mass) . |k_i|
    d k_i   = sum over the pixels of (the row's gradient) s_i         sum of (the row's mass) |s_i|

and every other result and mass is `compose`'s own.  `compose` rounds its inputs to float32: the colours and visibilities of
the cases are dyadic fractions (`dyadic`) whose products are exact in float32, which `compose` here asserts.

`torch_form` is the other route: `lighting.cook_torrance(..., visibility=)`, the ambient term, the mask composite and the clamp
on shared leaves, gradients by torch's autograd.  In float64 it must agree with the restatement; in float32 it is the
composition whose error sets the tolerance (`measure_f32`).

    python -m tests.shade_pbr_visibility_reference      # prints the float32 figures tests/test_shade_pbr_visibility.py restates
"""
import numpy as np
import torch

from dirt_amd import lighting
from tests import shade_pbr_reference as R
from tests.shade_reference import worst_ratio

KINDS = R.KINDS + ('d_visibility',)
COLOR_BITS, VISIBILITY_BITS = 6, 8      # 6 + 8 significant bits: a product is exact in float32


def dyadic(rng, lo, hi, shape, bits):
    """uniform multiples of 2^-bits in [lo, hi], float32"""
    return (rng.integers(int(np.ceil(lo * 2 ** bits)), int(np.floor(hi * 2 ** bits)) + 1, shape) / 2. ** bits).astype(np.float32)


def _rows(x, idx):
    """a parameter [3] or [R, 3] -> its row per pixel [N, 3], float32"""
    x = np.asarray(x, np.float32)
    return np.broadcast_to(x, (len(idx), 3)).copy() if x.ndim == 1 else x[idx]


def compose(gbuffer, lights, layout, visibility, scene_index=None, grad_out=None, masses=True, dtype=torch.float64, exact=True, **kw):
    """As `R.compose`, with visibility [N, L] (float32 values): -> its dict, d_params / mass_params in the parameters' own rows
    ([1, 3] or [scenes, 3]), and d_visibility / mass_visibility [N, L].  exact=False: k s may round to float32 (for the masses of
    a visibility that is not dyadic)."""
    n = gbuffer.shape[0]
    idx = np.zeros(n, np.int64) if scene_index is None else np.asarray(scene_index, np.int64)
    vis = np.asarray(visibility, np.float32)
    expand = lambda x: _rows(x, idx) if np.asarray(x).ndim == 2 else np.asarray(x, np.float32)   # noqa: E731
    px_lights, k_rows = [], []
    for i, (kind, vector, color) in enumerate(lights):
        k = _rows(color, idx)
        ks = k * vis[:, i:i + 1]
        assert not exact or np.array_equal(ks.astype(np.float64), k.astype(np.float64) * vis[:, i:i + 1].astype(np.float64)), 'k s is not exact in float32'
        px_lights.append((kind, expand(vector), ks))
        k_rows.append(k)
    kw = {k: expand(v) if k in ('ambient', 'background', 'camera_position') else v for k, v in kw.items()}
    res = R.compose(gbuffer, px_lights, layout, scene_index=np.arange(n), grad_out=grad_out, masses=masses, dtype=dtype, **kw)
    if grad_out is None:
        return res
    t_idx = torch.from_numpy(idx)
    rows = int(idx.max()) + 1 if n else 1
    originals = dict(zip(R.param_names(len(lights)), [kw.get('ambient', (0., 0., 0.)), kw.get('background', (0., 0., 0.)),
                                                      kw.get('camera_position', (0., 0., 4.))] + [x for rec in lights for x in rec[1:3]]))

    def fold(per_pixel, name):
        """the rows `R.compose` returned for a parameter -> the parameter's own rows"""
        if per_pixel.shape[0] != n:
            return per_pixel                                  # shared and not expanded: `R.compose` summed it
        shared = np.asarray(originals[name]).ndim == 1
        out = torch.zeros(1 if shared else rows, 3, dtype=per_pixel.dtype)
        return out.index_add_(0, torch.zeros_like(t_idx) if shared else t_idx, per_pixel)

    for prefix, absolute in (('d_', False),) + ((('mass_', True),) if masses else ()):
        params = res[prefix + 'params']
        cols = []
        for i in range(len(lights)):
            row = params['light%d.color' % i]
            k, s = torch.from_numpy(k_rows[i]).to(row.dtype), torch.from_numpy(vis[:, i:i + 1]).to(row.dtype)
            if absolute:
                k, s = k.abs(), s.abs()
            cols.append((row * k).sum(1))
            params['light%d.color' % i] = row * s
        res[prefix + 'visibility'] = torch.stack(cols, 1) if cols else torch.zeros(n, 0, dtype=res['out'].dtype)
        res[prefix + 'params'] = {name: fold(v, name) for name, v in params.items()}
    return res


def torch_form(gbuffer, lights, layout, visibility, colors=None, material=None, ambient=(0., 0., 0.), camera_position=(0., 0., 4.),
               background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04, grad_out=None, scene_index=None,
               dtype=torch.float32):
    """The composition a user writes with `lighting.cook_torrance(..., visibility=)`: same arguments and results as `compose`
    (without masses), the parameters as shared leaves [R, 3] indexed per pixel."""
    t = lambda x: R._t(x, dtype)   # noqa: E731
    g = t(gbuffer).requires_grad_(True)
    n = g.shape[0]
    idx = torch.zeros(n, dtype=torch.long) if scene_index is None else torch.as_tensor(np.asarray(scene_index)).long()
    col = t(colors).requires_grad_(True) if colors is not None else None
    mat = t(material).requires_grad_(True) if material is not None else None
    vis = t(visibility).requires_grad_(True)
    names = R.param_names(len(lights))
    values = [ambient, background, camera_position] + [x for rec in lights for x in rec[1:3]]
    leaves = {k: t(v).reshape(-1, 3).requires_grad_(True) for k, v in zip(names, values)}
    at = {k: v[idx if v.shape[0] > 1 else torch.zeros_like(idx)] for k, v in leaves.items()}
    sl = lambda k, w: g[:, layout[k]:layout[k] + w]   # noqa: E731
    c = col if col is not None else sl('colors', 3)
    rm = mat if mat is not None else sl('material', 2)
    m = sl('mask', 1) if layout.get('mask') is not None else torch.ones(n, 1, dtype=dtype)
    recs = [(rec[0], at['light%d.vector' % i], at['light%d.color' % i]) for i, rec in enumerate(lights)]
    lit = at['ambient'] * c + lighting.cook_torrance(sl('positions', 3)[:, None], sl('normals', 3)[:, None], c[:, None], rm[:, None, 0],
                                                     rm[:, None, 1], at['camera_position'], recs, min_roughness, dielectric_f0,
                                                     visibility=vis[:, None])[:, 0]
    pre = lit * m + at['background'] * (1. - m)
    out = torch.clamp(pre, clamp[0], clamp[1]) if clamp is not None else pre
    res = {'out': out.detach()}
    if grad_out is None:
        return res
    inputs = [g, vis] + [leaves[k] for k in names] + [x for x in (col, mat) if x is not None]
    grads = [torch.zeros_like(x) if gr is None else gr
             for x, gr in zip(inputs, torch.autograd.grad((out * t(grad_out)).sum(), inputs, allow_unused=True))]
    res['d_gbuffer'], res['d_visibility'] = grads[0], grads[1]
    for k, w in R.ATTRIBUTES:
        if layout.get(k) is not None:
            res['d_' + k] = grads[0][:, layout[k]:layout[k] + w]
    if col is not None:
        res['d_colors'] = grads[2 + len(names)]
    if mat is not None:
        res['d_material'] = grads[-1]
    res['d_params'] = dict(zip(names, grads[2:2 + len(names)]))
    return res


def ratios(got, ref):
    """`R.ratios`, and the visibility's gradient"""
    worst = R.ratios(got, ref)
    if got.get('d_visibility') is not None and 'd_visibility' in ref:
        a = np.asarray(got['d_visibility'].detach().cpu(), np.float64).reshape(ref['d_visibility'].shape)
        worst['d_visibility'] = worst_ratio(a, ref['d_visibility'].numpy(), ref['mass_visibility'].numpy())
    return worst


def measure_f32(cases):
    """cases: iterable of (positional arguments, keyword arguments) of `compose` -> the worst |f32 - f64| / mass of the float32
    torch form per kind of result (KINDS)."""
    worst = dict.fromkeys(KINDS, 0.)
    for args, kw in cases:
        r64 = compose(*args, dtype=torch.float64, **kw)
        r32 = torch_form(*args, dtype=torch.float32, **kw)
        for k, v in ratios(r32, r64).items():
            worst[k] = max(worst[k], v)
    return worst


if __name__ == '__main__':
    from tests import test_shade_pbr_visibility as T
    print({k: '%.3e' % v for k, v in measure_f32(T.case_of(name)[0].measure() for name in T.CASES).items()})
