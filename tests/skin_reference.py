"""The restatement `dirt_amd.skinning.skin_vertices` is checked against: linear-blend skinning composed from torch ops on CPU
tensors as DESIGN.md §7d says, gradients by torch's autograd.  Run in float64 it is the reference; run in float32 it is
the gather form users wrote before the kernel, whose error sets the tolerance (`measure_f32`).

    v4 = (x, y, z, w or 1)      M[v] = sum over k in slot order of w[v, k] * T[idx[v, k]]      posed[v] = (v4 @ M[v])[:3]

Beside every result it returns, per element, the L1 mass of the terms summed into that element: the scale an error of
that element is measured against.  Values and gradients come from the composition and autograd alone; only the masses
are written out here, in float64, as the same sums with every term replaced by its absolute value (A = sum over k of
|w| |T[idx]|, columns 0-2):

    posed          |v4| @ A                              d_vertices     |g| @ A^T                    (all 3 or 4 components)
    d_transforms   sum over the entries of a bone of |w| outer(|v4|, |g|), column 3 zero
    d_weights      (|v4| @ |T[idx]|)[:3] . |g|
an operand shared by the scenes carrying the sum over the scenes.

    python -m tests.skin_reference      # prints the float32 figures the constants of tests/test_skinning.py restate
"""
import numpy as np
import torch

VALUE_KINDS = ('posed',)
GRAD_KINDS = ('d_vertices', 'd_transforms', 'd_weights')


# ------------------------------------------------------------------------------------------------------------ inputs

def random_transforms(rng, num_bones, batch=None):
    """rotation x scale in [0.7, 1.3] + translation in row 3 (row-vector convention), and a last column a little off
    (0, 0, 0, 1): it is never read.  -> [J, 4, 4] or [batch, J, 4, 4] float32"""
    out = np.zeros((batch or 1, num_bones, 4, 4))
    for t in out.reshape(-1, 4, 4):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        t[:3, :3] = q * rng.uniform(0.7, 1.3)
        t[3, :3] = rng.uniform(-0.5, 0.5, 3)
        t[:, 3] = np.asarray([0., 0., 0., 1.]) + rng.uniform(-0.02, 0.02, 4)
    return np.asarray(out if batch else out[0], np.float32)


def random_weights(rng, num_vertices, influences, num_bones, root=False):
    """-> (bone_indices [V, K] int32, bone_weights [V, K] float32): random bones (repeats inside a vertex happen), positive
    weights normalised to one, about one slot in six a zero-weight padding.  root: slot 0 of every vertex names bone 0."""
    idx = rng.integers(0, num_bones, (num_vertices, influences)).astype(np.int32)
    if root:
        idx[:, 0] = 0
    w = rng.uniform(0.05, 1., (num_vertices, influences))
    w[rng.uniform(size=w.shape) < 1. / 6.] = 0.
    w[:, 0] = np.maximum(w[:, 0], 0.05)
    return idx, (w / w.sum(1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the restatement

def _t(x, dtype):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)


def compose(vertices, bone_indices, bone_weights, transforms, grad=None, dtype=torch.float64, masses=True):
    """vertices [V, 3|4] or [B, V, 3|4], bone_indices [V, K], bone_weights [V, K], transforms [J, 4, 4] or [B, J, 4, 4]
    (float32 values); grad: d loss / d posed, or None.
    -> dict of float tensors: posed; with `grad` also d_vertices, d_transforms, d_weights; with `masses` a 'mass_' + name
    beside each (float64 only)."""
    vertices, transforms = np.asarray(vertices, np.float32), np.asarray(transforms, np.float32)
    idx = torch.as_tensor(np.asarray(bone_indices)).long()
    v = _t(vertices, dtype).requires_grad_(True)
    T = _t(transforms, dtype).requires_grad_(True)
    w = _t(bone_weights, dtype).requires_grad_(True)
    K = idx.shape[1]
    v4 = v if v.shape[-1] == 4 else torch.cat([v, torch.ones_like(v[..., :1])], -1)

    def blend(Tm, wm):
        M = None
        for k in range(K):   # in slot order
            term = wm[:, k, None, None] * Tm[..., idx[:, k], :, :]
            M = term if M is None else M + term
        return M

    M = blend(T, w)                                                     # [.., V, 4, 4]
    posed = (v4[..., None, :] @ M)[..., 0, :3]
    res = {'posed': posed.detach()}
    batched = posed.dim() == 3
    if masses:
        assert dtype == torch.float64
        with torch.no_grad():
            A = blend(T.abs(), w.abs())[..., :3]                        # [.., V, 4, 3]
            res['mass_posed'] = (v4.abs()[..., None, :] @ A)[..., 0, :]
    if grad is None:
        return res
    g = _t(grad, dtype).reshape(posed.shape)
    for name, leaf, gr in zip(GRAD_KINDS, (v, T, w), torch.autograd.grad((posed * g).sum(), [v, T, w])):
        res[name] = gr
    if not masses:
        return res
    with torch.no_grad():
        ga, va = g.abs(), v4.abs()
        m_dv = (A @ ga[..., None])[..., 0][..., :v.shape[-1]]          # [.., V, C]
        res['mass_d_vertices'] = m_dv.sum(0) if batched and v.dim() == 2 else m_dv
        outer = (va[..., :, None] * ga[..., None, :]).expand(posed.shape[:-1] + (4, 3))   # [.., V, 4, 3]
        Bn = posed.shape[0] if batched else 1
        outer_b = outer.reshape(Bn, -1, 4, 3)
        m_dT = torch.zeros(Bn, T.shape[-3], 4, 4, dtype=dtype)
        for k in range(K):
            m_dT[..., :3] = m_dT[..., :3].index_add(1, idx[:, k], w.abs()[None, :, k, None, None] * outer_b)
        res['mass_d_transforms'] = (m_dT if T.dim() == 4 else m_dT.sum(0)).reshape(T.shape)
        m_dw = torch.zeros(Bn, idx.shape[0], K, dtype=dtype)
        Tb = T.abs().reshape(-1, T.shape[-3], 4, 4)
        for k in range(K):
            y = (va.reshape(-1, idx.shape[0], 4).expand(Bn, -1, -1)[..., None, :] @ Tb[:, idx[:, k]])[..., 0, :3]
            m_dw[..., k] = (y * ga.reshape(Bn, -1, 3)).sum(-1)
        res['mass_d_weights'] = m_dw.sum(0)
    return res


def worst_ratio(got, ref, mass):
    """max |got - ref| / mass over the elements with mass > 0 (0 if there are none)"""
    got, ref, mass = (np.asarray(x, dtype=np.float64) for x in (got, ref, mass))
    pos = (mass > 0) & np.isfinite(mass) & np.isfinite(ref)
    return float((np.abs(got - ref)[pos] / mass[pos]).max()) if pos.any() else 0.


def measure_f32(cases):
    """cases: iterable of keyword dicts for `compose` -> the worst |f32 - f64| / mass of the float32 composition per kind of
    result: {'posed', 'd_vertices', 'd_transforms', 'd_weights'}"""
    worst = {k: 0. for k in VALUE_KINDS + GRAD_KINDS}
    for kw in cases:
        r64 = compose(dtype=torch.float64, **kw)
        r32 = compose(dtype=torch.float32, masses=False, **kw)
        for k in worst:
            if r64.get(k) is not None:
                worst[k] = max(worst[k], worst_ratio(r32[k], r64[k], r64['mass_' + k]))
    return worst


if __name__ == '__main__':
    from tests import test_skinning
    for name, value in measure_f32(test_skinning.tolerance_cases()).items():
        print('%-20s %.3e' % (name, value))
