"""The restatement `dirt_amd.shading.resolve_image` (and its torch form `dirt_amd.lighting.resolve_image`) is checked against:
the specification of DESIGN.md §7j in numpy float64, written from the other end -- the box filter as one reshape and sum, the
curves' derivatives by hand, every gradient by hand -- so that it shares neither code nor order of operations with
`dirt_amd.lighting`.

The L1 mass of an element is the sum of the absolute values of the terms it is added up from.  The mass of L is the mean of
its samples' absolute values (|image| + |add|); from there the masses follow the chain rule with every factor's absolute
value: E = e L has |e| mass(L), a floored value none, t = curve(x) has |curve'(x)| mass(x), the linear sRGB segment 12.92
mass(u), the upper one counts 1.055 pow and 0.055 as two terms, (1.055 / 2.4) u^(1/2.4 - 1) mass(u) + 0.055, and a clamped
value is a constant: no mass.  A gradient is a product g * slopes, whose mass is the product of the absolute values, with the
two differences inside the curves' derivatives ((1 + 2x/w^2)(1 + x) - a for Reinhard, n' q - n q' for ACES) counted as sums; the
exposure's and the white point's gradients are sums over pixels (and over the scenes where shared) of such products.  An
element whose mass is zero must be exact.

The kink measure of an element: |E| < OFF_KINKS where the curve or the encoding floors, |u - knee| < OFF_KINKS with 'srgb',
|y - lo| or |y - hi| < OFF_KINKS under a clamp (on the value before the clamp, and only where E > 0).  Elements on a kink are not
compared and carry a zero incoming gradient, so that they add to no sum.

The float32 torch form run on the same inputs is what a user had before the kernel; its worst |f32 - ref64| / mass per kind
of result sets the tolerance:

    python -m tests.resolve_reference      # prints the float32 figures the F32 table of tests/test_resolve.py restates
"""
import functools

import numpy as np
import torch

from tests.shade_reference import worst_ratio

KINDS = ('out', 'd_image', 'd_add', 'd_exposure', 'd_white')
OFF_KINKS = 1.e-4
KNEE = 0.0031308
EXPOSURE = (0.9, 1.2, 0.8, 1.1)     # the first C of them
WHITE = 2.


def _curve(x, curve, w):
    """t, dt/dx and its mass, dt/dw of a tone curve at x >= 0"""
    if curve == 'reinhard':
        ww, b = w * w, 1. + x
        a = x * (1. + x / ww)
        return a / b, ((1. + 2. * x / ww) * b - a) / (b * b), ((1. + 2. * x / ww) * b + a) / (b * b), -2. * x * x / (ww * w * b)
    n, q = x * (2.51 * x + 0.03), x * (2.43 * x + 0.59) + 0.14
    dn, dq = 5.02 * x + 0.03, 4.86 * x + 0.59
    return n / q, (dn * q - n * dq) / (q * q), (dn * q + n * dq) / (q * q), np.zeros_like(x)


def compose(image, add=None, factor=1, exposure=1.0, curve='linear', white=None, encode='linear', clamp=(0., 1.), grad_out=None):
    """-> dict: out, kink (bool), E, t, pre (y before the clamp), mass_out, and with grad_out: d_image, d_add, d_exposure, d_white
    with mass_d_*, each shaped like its operand (a number's like a 0-d array)."""
    S = int(factor)
    img, ad = np.asarray(image, np.float64), None if add is None else np.asarray(add, np.float64)
    e, w = np.asarray(exposure, np.float64), None if white is None else np.asarray(white, np.float64)
    lead = [x.shape[0] for x, rank in ((img, 4), (e, 2)) if x.ndim == rank] + ([w.shape[0]] if w is not None and w.ndim == 1 else [])
    B = lead[0] if lead else None
    img4 = img if img.ndim == 4 else img[None]
    ad4 = None if ad is None else (ad if ad.ndim == 4 else ad[None])
    n, SH, SW, C = img4.shape
    H, W = SH // S, SW // S
    box = lambda x: x.reshape(n, H, S, W, S, C).sum((2, 4)) / (S * S)   # noqa: E731
    L = box(img4 if ad4 is None else img4 + ad4)
    mass_L = box(np.abs(img4) if ad4 is None else np.abs(img4) + np.abs(ad4))
    eb = e.reshape((-1, 1, 1, C)) if e.ndim else e.reshape(1, 1, 1, 1)
    wb = None if w is None else w.reshape(-1, 1, 1, 1)
    full = np.broadcast_shapes((eb * L).shape, (B or 1, 1, 1, 1))
    E = np.broadcast_to(eb * L, full)
    mass_E = np.abs(eb) * mass_L
    kink = np.zeros(full, bool)
    if curve == 'linear':
        t, dt, mdt, dtw = E, np.ones(full), np.ones(full), np.zeros(full)
    else:
        x = np.maximum(E, 0.)
        t, dt, mdt, dtw = (np.broadcast_to(v, full) for v in _curve(x, curve, wb))
        live = E > 0
        dt, mdt, dtw = dt * live, mdt * live, dtw * live
        kink |= np.abs(E) < OFF_KINKS
    mass_t = mdt * mass_E
    if encode == 'srgb':
        u = np.maximum(t, 0.)
        upper = u > KNEE
        p = np.where(upper, u, 1.) ** (1. / 2.4)
        pre = np.where(upper, 1.055 * p - 0.055, 12.92 * u)
        slope = np.where(upper, (1.055 / 2.4) * p / np.where(upper, u, 1.), 12.92) * (t > 0)
        mass_pre = np.where(upper, slope * mass_t + 0.055, 12.92 * mass_t) * (t > 0)
        kink |= (np.abs(u - KNEE) < OFF_KINKS) | (np.abs(E) < OFF_KINKS)      # (with the linear curve the encoding floors)
    else:
        pre, slope, mass_pre = t, np.ones(full), mass_t
    if clamp is not None:
        lo, hi = (float(np.float32(v)) for v in clamp)
        out = np.clip(pre, lo, hi)
        inside = (pre >= lo) & (pre <= hi)
        kink |= ((np.abs(pre - lo) < OFF_KINKS) | (np.abs(pre - hi) < OFF_KINKS)) & (E > 0)
    else:
        out, inside = pre, np.ones(full, bool)
    shape_out = full if B is not None else full[1:]
    res = {'out': out.reshape(shape_out), 'mass_out': (mass_pre * inside).reshape(shape_out), 'kink': kink.reshape(shape_out),
           'E': E.reshape(shape_out), 't': np.broadcast_to(t, full).reshape(shape_out), 'pre': pre.reshape(shape_out)}
    if grad_out is None:
        return res
    g = np.asarray(grad_out, np.float64).reshape(full)
    gt, mgt = g * inside * slope, np.abs(g) * inside * slope
    gE, mgE = gt * dt, mgt * mdt
    spread = lambda x: np.repeat(np.repeat(x, S, 1), S, 2) / (S * S)   # noqa: E731
    d_samples, m_samples = spread(gE * eb), spread(mgE * np.abs(eb))
    for name, operand in (('image', img), ('add', ad)):
        if operand is not None:
            shared = operand.ndim == 3
            res['d_' + name] = d_samples.sum(0) if shared else d_samples
            res['mass_d_' + name] = m_samples.sum(0) if shared else m_samples
    de, mde = (gE * L).sum((1, 2)), (mgE * mass_L).sum((1, 2))            # [B or 1, C]
    if e.ndim == 2:
        res['d_exposure'], res['mass_d_exposure'] = de, mde
    elif e.ndim == 1:
        res['d_exposure'], res['mass_d_exposure'] = de.sum(0), mde.sum(0)
    else:
        res['d_exposure'], res['mass_d_exposure'] = de.sum(), mde.sum()
    if w is not None:
        dw, mdw = (gt * dtw).sum((1, 2, 3)), (mgt * np.abs(dtw)).sum((1, 2, 3))
        res['d_white'], res['mass_d_white'] = (dw, mdw) if w.ndim == 1 else (dw.sum(), mdw.sum())
    return res


def torch_form(image, add=None, grad_out=None, dtype=torch.float32, device='cpu', function=None, **kw):
    """The same results (no masses) from `lighting.resolve_image` -- or `function`, the fused call -- and torch's autograd; a number
    stays a number and has no gradient."""
    from dirt_amd import lighting
    leaf = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype, device=device, requires_grad=True)   # noqa: E731
    img, ad = leaf(image), leaf(add)
    e = kw['exposure'] if np.ndim(kw['exposure']) == 0 and not isinstance(kw['exposure'], np.ndarray) else leaf(kw['exposure'])
    w = kw.get('white')
    w = w if w is None or not isinstance(w, np.ndarray) else leaf(w)
    out = (function or lighting.resolve_image)(img, add=ad, **dict(kw, exposure=e, white=w))
    res = {'out': out.detach().cpu().numpy()}
    if grad_out is not None:
        out.backward(torch.tensor(np.asarray(grad_out), dtype=dtype, device=device))
        for name, x in (('d_image', img), ('d_add', ad), ('d_exposure', e), ('d_white', w)):
            if isinstance(x, torch.Tensor):
                res[name] = x.grad.cpu().numpy()
    return res


def ratios(got, ref):
    """the worst |got - ref| / mass per kind of result that `got` has; the output off the kinks alone"""
    worst = {}
    for kind in KINDS:
        if kind in got and kind in ref:
            mass = ref['mass_' + kind] * ~ref['kink'] if kind == 'out' else ref['mass_' + kind]
            worst[kind] = worst_ratio(got[kind], ref[kind], mass)
    return worst


def exact_where_massless(got, ref):
    for kind in KINDS:
        if kind in got and kind in ref:
            dead = (np.asarray(ref['mass_' + kind]) == 0) & (~ref['kink'] if kind == 'out' else True)
            if not np.array_equal(np.asarray(got[kind], np.float64)[dead], np.asarray(ref[kind])[dead]):
                return False
    return True


# ---- the inputs

def samples(rng, shape, S):
    """[..., S H, S W, C] float64: per output pixel and channel a base value -- 20 % in (-0.3, 0), 10 % in (0, 0.004), 50 % in
    (0, 1), 20 % in (1, 12) --, each of its S x S samples the base times 1 + uniform(-0.2, 0.2)"""
    *lead, H, W, C = shape
    kind = rng.uniform(0., 1., shape)
    lo = np.select([kind < 0.2, kind < 0.3, kind < 0.8], [-0.3, 0., 0.], 1.)
    hi = np.select([kind < 0.2, kind < 0.3, kind < 0.8], [0., 0.004, 1.], 12.)
    base = lo + (hi - lo) * rng.uniform(0., 1., shape)
    fine = np.repeat(np.repeat(base, S, -3), S, -2)
    return fine * (1. + rng.uniform(-0.2, 0.2, fine.shape))


class Case:
    """One call: image and add (float32; a sample split 0.75 / 0.25 between them), the keywords, and an incoming gradient with
    zeros on the kinks.  batch: None or B; image_scene (image and add) / exposure_scene / white_scene: whether the operand has a leading B;
    exposure 'tensor' or 'number', white likewise."""

    def __init__(self, seed, S=2, curve='aces', encode='srgb', C=3, size=(17, 19), add=True, clamp=(0., 1.), batch=None, image_scene=True,
                 exposure='tensor', exposure_scene=False, white='tensor', white_scene=False):
        rng = np.random.default_rng(seed)
        lead = lambda scene: (batch,) if batch is not None and scene else ()   # noqa: E731
        x = samples(rng, lead(image_scene) + tuple(size) + (C,), S)
        self.image = (x * (0.75 if add else 1.)).astype(np.float32)
        self.add = None
        if add:
            self.add = (0.25 * x).astype(np.float32)
        if exposure == 'number':
            e = 1.1
        else:
            e = np.asarray(EXPOSURE[:C], np.float32)
            if batch is not None and exposure_scene:
                e = (e[None] * (1. + 0.15 * np.arange(batch))[:, None]).astype(np.float32)
        w = None
        if curve == 'reinhard':
            w = WHITE if white == 'number' else np.asarray(WHITE, np.float32)
            if white != 'number' and batch is not None and white_scene:
                w = (WHITE + 0.5 * np.arange(batch)).astype(np.float32)
        self.kw = dict(factor=S, exposure=e, curve=curve, white=w, encode=encode, clamp=clamp)
        first = compose(self.image, self.add, **self.kw)
        self.go = (np.random.default_rng(seed + 1).standard_normal(first['out'].shape) * ~first['kink']).astype(np.float32)

    @functools.cached_property
    def ref(self):
        return compose(self.image, self.add, grad_out=self.go, **self.kw)

    @property
    def share(self):
        return float(self.ref['kink'].mean())

    def classes(self):
        """how many elements off the kinks are floored, on the linear sRGB segment, above 1 before the clamp, inside"""
        r = self.ref
        keep = ~r['kink']
        return {'floored': int((keep & (r['E'] < 0)).sum()), 'segment': int((keep & (r['t'] > 0) & (r['t'] <= KNEE)).sum()),
                'above': int((keep & (r['pre'] > 1)).sum()), 'inside': int((keep & (r['t'] > KNEE) & (r['pre'] < 1)).sum())}


CURVES, ENCODINGS = ('linear', 'reinhard', 'aces'), ('linear', 'srgb')
GRID = ['grid-%d-%s-%s' % (S, c, e) for S in (1, 2, 3, 4) for c in CURVES for e in ENCODINGS]
# every mix of shared and per-scene operands with B = 3 (image and add, exposure, white): at least one per scene
MIXES = ['batch-%d%d%d' % m for m in [(1, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]]
OTHERS = ['channels-1-2', 'channels-1-3', 'channels-4-2', 'channels-4-3', 'no-add-2', 'no-add-3', 'clamp-none', 'clamp-none-linear', 'clamp-inner',
          'clamp-inner-reinhard', 'numbers', 'numbers-batch']
# where the kernels' walk can go wrong whatever a workgroup's span: one output pixel (the sums have a single term: their worst
# case relative to the mass), rows of 1, 2 and 3 floats modulo 4
SMALL = ['pixel-%d' % S for S in (1, 2, 3, 4)] + ['row-%d-%d-%d' % (W, S, C) for W in (17, 18, 19, 20) for S in (1, 2, 3) for C in (1, 3)]
NAMES = GRID + MIXES + OTHERS + SMALL


@functools.lru_cache(maxsize=None)
def case(name):
    k = NAMES.index(name)
    part = name.split('-')
    if part[0] == 'grid':
        return Case(100 + k, S=int(part[1]), curve=part[2], encode=part[3])
    if part[0] == 'batch':
        i, e, w = (c == '1' for c in part[1])
        return Case(100 + k, S=2 + k % 2, curve='reinhard', batch=3, image_scene=i, exposure_scene=e, white_scene=w)
    if part[0] == 'channels':
        return Case(100 + k, S=int(part[2]), C=int(part[1]), curve=('aces', 'reinhard')[k % 2])
    if part[0] == 'no':
        return Case(100 + k, S=int(part[2]), add=False, curve=('aces', 'linear')[k % 2], encode=('srgb', 'linear')[k % 2])
    if part[0] == 'pixel':
        return Case(100 + k, S=int(part[1]), size=(1, 1), curve=('aces', 'reinhard')[k % 2])
    if part[0] == 'row':
        return Case(100 + k, S=int(part[2]), size=(12, int(part[1])), C=int(part[3]), curve=('aces', 'reinhard')[k % 2])
    if name == 'clamp-none':
        return Case(100 + k, clamp=None)
    if name == 'clamp-none-linear':
        return Case(100 + k, clamp=None, curve='linear', encode='linear', S=3)
    if name == 'clamp-inner':
        return Case(100 + k, clamp=(0.1, 0.8))
    if name == 'clamp-inner-reinhard':
        return Case(100 + k, clamp=(0.1, 0.8), curve='reinhard', encode='linear', S=4)
    if name == 'numbers':
        return Case(100 + k, curve='reinhard', exposure='number', white='number')
    if name == 'numbers-batch':
        return Case(100 + k, curve='reinhard', exposure='number', white='number', batch=3, S=3)
    raise KeyError(name)


def measure_f32(names=NAMES):
    worst = dict.fromkeys(KINDS, 0.)
    for name in names:
        c = case(name)
        for kind, x in ratios(torch_form(c.image, c.add, c.go, **c.kw), c.ref).items():
            worst[kind] = max(worst[kind], x)
    return worst


if __name__ == '__main__':
    import math
    up = lambda v: math.ceil(v / 10. ** (math.floor(math.log10(v)) - 2)) * 10. ** (math.floor(math.log10(v)) - 2)   # noqa: E731  (three digits, rounded up)
    print({k: float('%.3g' % up(v)) for k, v in measure_f32().items()})
    full = [n for n in NAMES if not n.startswith('pixel')]
    shares, least = [case(n).share for n in full], [min(case(n).classes().values()) for n in full]
    print('worst share left out %.4f, smallest class %d' % (max(shares), min(least)))
