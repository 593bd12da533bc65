"""The restatement `dirt_amd.kinematics.pose_skeleton` is checked against: the forward kinematics of a skeleton composed from
torch ops on CPU tensors as DESIGN.md §7e says, gradients by torch's autograd.  Run in float64 it is the reference; run in
float32 it is what users wrote before the kernel, whose error sets the tolerance (`measure_f32`).

    R[j]  = matrices.rodrigues(r[j], three_by_three=True)           tl[j] = p[j] - p[j] @ R[j]
    root:   S3[j] = R[j],                 t[j] = tl[j]
    else:   S3[j] = R[j] @ S3[parent],    t[j] = tl[j] @ S3[parent] + t[parent]
    transforms[j] = [[S3[j], 0], [t[j], 1]]                         posed_joints[j] = p[j] @ S3[j] + t[j]

Beside every result it returns, per element, the L1 mass of the terms summed into that element: the scale an error of
that element is measured against.  Values and gradients come from the composition and autograd alone; only the masses
are written out here, in float64, as the same recursion with every term replaced by its absolute value:

    values      mR = |c| I + |1 - c| |k k^T| + |s| |K|  (by term, not |R|: a zero rotation's off-diagonal elements are
                s K alone), m_tl = |p| + |p| @ mR, then mS3, mt and the posed joints by the recursion above; column 3 of
                the transforms has no mass: it is (0, 0, 0, 1) to the bit
    gradients   the reverse recursion from the seeds |gT| and |gq| through |R|^T and |S3|^T, down to m_dR and d_joints;
                d_rotations = (the absolute float64 Jacobian of rodrigues, by torch.autograd.functional.jacobian) applied to m_dR
an operand shared by the scenes carrying the sum over the scenes.

`loop` is the composition as examples/fit_pose_fused.py writes it -- rodrigues, two translations and up to three compose
per joint -- generalised from a chain to a tree.

    python -m tests.kinematics_reference      # prints the float32 figures the constants of tests/test_kinematics.py restate
"""
import numpy as np
import torch

from dirt_amd import matrices

VALUE_KINDS = ('transforms', 'posed_joints')
GRAD_KINDS = ('d_rotations', 'd_joints')

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)   # the 24-joint SMPL body


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)


def _row(x, M):
    """row vectors [.., 3] times matrices [.., 3, 3]"""
    return (x[..., None, :] @ M)[..., 0, :]


def walk(R, tl, parents, lead):
    """the recursion over the tree: R [.., J, 3, 3], tl [.., J, 3] -> S3 [lead, J, 3, 3], t [lead, J, 3]"""
    S3, t = [], []
    for j, q in enumerate(parents):
        if q < 0:
            S3.append(R[..., j, :, :])
            t.append(tl[..., j, :])
        else:
            S3.append(R[..., j, :, :] @ S3[q])
            t.append(_row(tl[..., j, :], S3[q]) + t[q])
    return (torch.stack([x.expand(lead + (3, 3)) for x in S3], -3), torch.stack([x.expand(lead + (3,)) for x in t], -2))


def loop(rotations, joints, parents):
    """What users wrote before the kernel (examples/fit_pose_fused.py: bone_transforms, for a tree): -> (transforms [.., J, 4, 4],
    posed_joints [.., J, 3]), on the device and in the dtype of the inputs"""
    out = []
    for j, q in enumerate(parents):
        pivot = joints[..., j, :]
        local = matrices.compose(matrices.translation(-pivot), matrices.rodrigues(rotations[..., j, :]), matrices.translation(pivot))
        out.append(local if q < 0 else matrices.compose(local, out[q]))
    lead = torch.broadcast_shapes(rotations.shape[:-2], joints.shape[:-2])
    T = torch.stack([x.expand(lead + (4, 4)) for x in out], -3)
    p4 = torch.cat([joints, torch.ones_like(joints[..., :1])], -1)
    return T, (p4[..., None, :] @ T)[..., 0, :3]


def compose(rotations, joints, parents, grad_transforms=None, grad_posed_joints=None, dtype=torch.float64, masses=True):
    """rotations, joints [J, 3] or [B, J, 3] (float32 values), parents: a sequence; grad_transforms [.., J, 4, 4] and
    grad_posed_joints [.., J, 3]: d loss / d output, or None (the output is not used).
    -> dict of float tensors: transforms, posed_joints; with a gradient also d_rotations, d_joints; with `masses` a
    'mass_' + name beside each (float64 only)."""
    parents = [int(q) for q in parents]
    J = len(parents)
    r = _t(rotations, dtype).requires_grad_(True)
    p = _t(joints, dtype).requires_grad_(True)
    lead = torch.broadcast_shapes(r.shape[:-2], p.shape[:-2])
    R = matrices.rodrigues(r, three_by_three=True)
    tl = p - _row(p, R)
    S3, t = walk(R, tl, parents, lead)
    zeros, ones = torch.zeros(lead + (J, 3, 1), dtype=dtype), torch.ones(lead + (J, 1, 1), dtype=dtype)
    T = torch.cat([torch.cat([S3, zeros], -1), torch.cat([t[..., None, :], ones], -1)], -2)
    posed = _row(p, S3) + t
    res = {'transforms': T.detach(), 'posed_joints': posed.detach()}
    if masses:
        assert dtype == torch.float64
        with torch.no_grad():
            rb, pa = r.expand(lead + (J, 3)), p.abs().expand(lead + (J, 3))
            v = rb + 1.e-12
            n = torch.linalg.vector_norm(v, dim=-1, keepdim=True)
            k = (v / n).abs()
            c, s = torch.cos(n)[..., None], torch.sin(n)[..., None]
            z = torch.zeros_like(k[..., 0])
            Ka = torch.stack([torch.stack([z, k[..., 2], k[..., 1]], -1), torch.stack([k[..., 2], z, k[..., 0]], -1),
                              torch.stack([k[..., 1], k[..., 0], z], -1)], -2)
            mR = c.abs() * torch.eye(3, dtype=dtype) + (1 - c).abs() * k[..., :, None] * k[..., None, :] + s.abs() * Ka
            mS3, mt = walk(mR, pa + _row(pa, mR), parents, lead)
            res['mass_transforms'] = torch.cat([torch.cat([mS3, zeros], -1), torch.cat([mt[..., None, :], torch.zeros_like(ones)], -1)], -2)
            res['mass_posed_joints'] = _row(pa, mS3) + mt
    if grad_transforms is None and grad_posed_joints is None:
        return res
    gT = None if grad_transforms is None else _t(grad_transforms, dtype).reshape(T.shape)
    gq = None if grad_posed_joints is None else _t(grad_posed_joints, dtype).reshape(posed.shape)
    loss = sum((out * g).sum() for out, g in ((T, gT), (posed, gq)) if g is not None)
    res['d_rotations'], res['d_joints'] = torch.autograd.grad(loss, [r, p])
    if not masses:
        return res
    with torch.no_grad():
        Ra, S3a, tla = R.detach().abs().expand(lead + (J, 3, 3)), S3.detach().abs(), tl.detach().abs().expand(lead + (J, 3))
        gTa = torch.zeros_like(T) if gT is None else gT.abs()
        gqa = torch.zeros_like(posed) if gq is None else gq.abs()
        mGS = [gTa[..., j, :3, :3] + pa[..., j, :, None] * gqa[..., j, None, :] for j in range(J)]
        mGt = [gTa[..., j, 3, :3] + gqa[..., j, :] for j in range(J)]
        m_dp = [(S3a[..., j, :, :] @ gqa[..., j, :, None])[..., 0] for j in range(J)]
        m_dR = [None] * J
        for j in range(J - 1, -1, -1):   # children before their parents
            q = parents[j]
            if q < 0:
                m_dR[j], m_dtl = mGS[j], mGt[j]
            else:
                SpT = S3a[..., q, :, :].transpose(-1, -2)
                m_dR[j], m_dtl = mGS[j] @ SpT, _row(mGt[j], SpT)
                mGS[q] = mGS[q] + Ra[..., j, :, :].transpose(-1, -2) @ mGS[j] + tla[..., j, :, None] * mGt[j][..., None, :]
                mGt[q] = mGt[q] + mGt[j]
            m_dp[j] = m_dp[j] + m_dtl + (Ra[..., j, :, :] @ m_dtl[..., None])[..., 0]
            m_dR[j] = m_dR[j] + pa[..., j, :, None] * m_dtl[..., None, :]
        m_dp, m_dR = torch.stack(m_dp, -2), torch.stack(m_dR, -3)
        flat = rb.detach().reshape(-1, 3)
        jac = torch.autograd.functional.jacobian(lambda x: matrices.rodrigues(x, three_by_three=True).sum(0), flat)   # [3, 3, N, 3]
        m_dr = torch.einsum('abni,nab->ni', jac.abs(), m_dR.reshape(-1, 3, 3)).reshape(lead + (J, 3))
        res['mass_d_rotations'] = m_dr.sum(0) if lead and r.dim() == 2 else m_dr
        res['mass_d_joints'] = m_dp.sum(0) if lead and p.dim() == 2 else m_dp
    return res


def worst_ratio(got, ref, mass):
    """max |got - ref| / mass over the elements with mass > 0 (0 if there are none)"""
    got, ref, mass = (np.asarray(x, dtype=np.float64) for x in (got, ref, mass))
    pos = (mass > 0) & np.isfinite(mass) & np.isfinite(ref)
    return float((np.abs(got - ref)[pos] / mass[pos]).max()) if pos.any() else 0.


def measure_f32(cases):
    """cases: iterable of keyword dicts for `compose` -> the worst |f32 - f64| / mass of the float32 composition per kind of
    result: {'transforms', 'posed_joints', 'd_rotations', 'd_joints'}"""
    worst = {k: 0. for k in VALUE_KINDS + GRAD_KINDS}
    for kw in cases:
        r64 = compose(dtype=torch.float64, **kw)
        r32 = compose(dtype=torch.float32, masses=False, **kw)
        for k in worst:
            if r64.get(k) is not None:
                worst[k] = max(worst[k], worst_ratio(r32[k], r64[k], r64['mass_' + k]))
    return worst


if __name__ == '__main__':
    from tests import test_kinematics
    for name, value in measure_f32(test_kinematics.tolerance_cases()).items():
        print('%-20s %.3e' % (name, value))
