"""CPU restatement (numpy) of the texture look-up of the reference's samples/textured.py -- TEST INFRASTRUCTURE: only
tests/ may import it; dirt_amd never does.

`sample_texture_uv` follows `uvs_to_pixel_indices` (samples/textured.py:16-26) and `sample_texture`
(samples/textured.py:29-60) operation for operation in float32; `sample_texture_uv_grad` is the analytic gradient of that
expression, accumulated in float64.  Where the reference's gather_nd would read row Ht / column Wt (an index inside the
last texel) the last texel is used (a documented choice of this build; TF's GPU gather_nd returns zeros there, its CPU
kernel raises).  Parity: the reference ships no expected values for its samples; these functions are pinned by the
reference's own two functions executed over a numpy stand-in for TensorFlow (tests/test_helpers_ref.py, committed
vectors tests/golden/helpers_ref.npz: equal wherever the reference's gather_nd stays inside the texture) and by the
analytic cases in tests/test_texture.py (texel centres, linear ramps)."""
import numpy as np


def _indices(uvs, ht, wt, mode):
    uvs = np.asarray(uvs, np.float32)[..., ::-1]                       # :20 x, y coordinates -> y, x indices
    shape = np.array([ht, wt], np.float32)
    with np.errstate(invalid='ignore'):                                # (inf - floor(inf): NaN, as in TF)
        if mode == 'repeat':
            return ((uvs - np.floor(uvs)).astype(np.float32) * shape).astype(np.float32)   # :22 uvs % 1. * texture_shape
        if mode == 'clamp':
            return (np.clip(uvs, np.float32(0), np.float32(1)) * shape).astype(np.float32)  # :24 (NaN stays NaN)
    raise NotImplementedError(mode)


def _int(x):
    """float -> int64 truncation; NaN -> 0 (what the kernels' conversion gives; the index is clamped afterwards)."""
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(x), x, 0.0).astype(np.int64)


def sample_texture_uv(texture, uvs, mode='repeat', filter='bilinear'):
    texture = np.asarray(texture, np.float32)
    ht, wt = texture.shape[:2]
    idx = _indices(uvs, ht, wt, mode)
    if filter == 'nearest':
        r = np.clip(_int(idx[..., 0]), 0, ht - 1)                        # :33 tf.cast(indices, tf.int32): truncation
        c = np.clip(_int(idx[..., 1]), 0, wt - 1)
        return texture[r, c]
    fl = np.floor(idx)                                                   # :37
    frac = (idx - fl).astype(np.float32)                                 # :38
    r0 = np.clip(_int(fl[..., 0]), 0, ht - 1)
    c0 = np.clip(_int(fl[..., 1]), 0, wt - 1)
    r1, c1 = np.minimum(r0 + 1, ht - 1), np.minimum(c0 + 1, wt - 1)
    fr, fc = frac[..., :1], frac[..., 1:]
    one = np.float32(1)
    tl, tr, bl, br = texture[r0, c0], texture[r0, c1], texture[r1, c0], texture[r1, c1]
    return (((tl * (one - fc)) * (one - fr) + (tr * fc) * (one - fr)) + (bl * (one - fc)) * fr) + (br * fc) * fr   # :53-57


def _taps(idx2, ht, wt):
    """Rows / columns of the four bilinear taps and the fractions, from float64 indices [n, 2].  A NaN index takes row /
    column 0 (and its NaN fraction makes every weight NaN), as the kernels' float -> int conversion does."""
    fl = np.floor(idx2)
    frac = idx2 - fl
    r0 = np.clip(_int(fl[:, 0]), 0, ht - 1); c0 = np.clip(_int(fl[:, 1]), 0, wt - 1)
    return r0, np.minimum(r0 + 1, ht - 1), c0, np.minimum(c0 + 1, wt - 1), frac[:, 0], frac[:, 1]


def sample_texture_uv_grad(texture, uvs, grad_out, mode='repeat', filter='bilinear', want_mass=False):
    """-> (grad_texture [Ht,Wt,C], grad_uvs [*,2]) of the look-up, float64 accumulation, returned as float32.

    `filter='nearest'`: the gradient of a gather -- every look-up's grad_out added into the one texel it read (the truncated
    index, as `sample_texture_uv`), and zero grad_uvs (tf.cast to int32 has no gradient).

    `want_mass=True` returns (grad_texture, grad_uvs, mass_texture, mass_uvs), all float64: the L1 mass of the terms added
    into each element -- per texel and channel sum |g * w| over the look-ups that touch it; per coordinate the terms of
    d_fc * dcol_du (u) and d_fr * drow_dv (v) with the texel differences taken over magnitudes (|t_tr| + |t_tl| for
    t_tr - t_tl), the cancellation scale, as cond_vertices in tests/parity.py.  A kernel's float32 sums of the same terms
    differ from these values by a small multiple of 2^-24 of the mass.

    Non-finite coordinates (the rule of samples/textured.py, whose tf.clip_by_value and floor-mod propagate NaN): `repeat`
    maps NaN and +-inf to a NaN index; `clamp` maps +-inf to the border and NaN to a NaN index.  A NaN index reads row /
    column 0 with NaN weights: the look-up and the gradients of its four texels are NaN; in `clamp` mode the coordinate's
    own gradient is 0 * (finite) where the clip is saturated (NaN is outside [0, 1]), NaN through the other coordinate's
    NaN fraction."""
    texture = np.asarray(texture, np.float64)
    ht, wt, ct = texture.shape
    uvs32 = np.asarray(uvs, np.float32)
    idx = _indices(uvs32, ht, wt, mode).astype(np.float64)
    g = np.asarray(grad_out, np.float64).reshape(-1, ct)
    idx2 = idx.reshape(-1, 2)
    gt = np.zeros_like(texture)
    mt = np.zeros_like(texture)
    if filter == 'nearest':
        r, c = np.clip(_int(idx2[:, 0]), 0, ht - 1), np.clip(_int(idx2[:, 1]), 0, wt - 1)
        np.add.at(gt, (r, c), g)
        np.add.at(mt, (r, c), np.abs(g))
        guv = np.zeros(uvs32.shape, np.float32)
        if want_mass:
            return gt.astype(np.float32), guv, mt, np.zeros(uvs32.shape, np.float64)
        return gt.astype(np.float32), guv
    if filter != 'bilinear':
        raise NotImplementedError(filter)
    r0, r1, c0, c1, fr, fc = _taps(idx2, ht, wt)
    for (rr, cc, w) in ((r0, c0, (1 - fc) * (1 - fr)), (r0, c1, fc * (1 - fr)), (r1, c0, (1 - fc) * fr), (r1, c1, fc * fr)):
        np.add.at(gt, (rr, cc), g * w[:, None])
        np.add.at(mt, (rr, cc), np.abs(g * w[:, None]))
    tl, tr, bl, br = texture[r0, c0], texture[r0, c1], texture[r1, c0], texture[r1, c1]
    d_fr = (g * ((bl - tl) * (1 - fc)[:, None] + (br - tr) * fc[:, None])).sum(-1)
    d_fc = (g * ((tr - tl) * (1 - fr)[:, None] + (br - bl) * fr[:, None])).sum(-1)
    u, v = uvs32.reshape(-1, 2)[:, 0], uvs32.reshape(-1, 2)[:, 1]
    if mode == 'clamp':
        du = np.where((u >= 0) & (u <= 1), wt, 0.0); dv = np.where((v >= 0) & (v <= 1), ht, 0.0)
    else:
        du = np.full_like(d_fc, wt); dv = np.full_like(d_fr, ht)
    guv = np.stack([d_fc * du, d_fr * dv], -1).reshape(uvs32.shape)
    if not want_mass:
        return gt.astype(np.float32), guv.astype(np.float32)
    a = np.abs
    m_fr = (a(g) * ((a(bl) + a(tl)) * a(1 - fc)[:, None] + (a(br) + a(tr)) * a(fc)[:, None])).sum(-1)
    m_fc = (a(g) * ((a(tr) + a(tl)) * a(1 - fr)[:, None] + (a(br) + a(bl)) * a(fr)[:, None])).sum(-1)
    muv = np.stack([m_fc * du, m_fr * dv], -1).reshape(uvs32.shape)
    return gt.astype(np.float32), guv.astype(np.float32), mt, muv
