"""`shading.resolve_image` (dirt_resolve.hip) against its torch form `lighting.resolve_image`, by the method of the fused stages:
tests/resolve_reference.py restates the specification of DESIGN.md §7j in float64; the float32 torch form's worst
|f32 - ref64| / mass per kind of result over the cases of `resolve_reference.NAMES` is the F32 table below (`python -m
tests.resolve_reference` prints it), and the kernel gets KERNEL times that, per element against the element's L1 mass.  An
element of zero mass -- a floored value, a clamped one -- must be exact.  Elements within 1e-4 of a kink (the floor, the knee of
the sRGB curve, a clamp bound), judged by the float64 values alone, are not compared and carry a zero incoming gradient."""
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import resolve_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python -m tests.resolve_reference
F32 = {'out': 3.93e-7, 'd_image': 4.49e-7, 'd_add': 4.49e-7, 'd_exposure': 1.21e-7, 'd_white': 1.17e-7}
KERNEL = 4     # the kernel's allowance over the float32 torch form

_SOURCE = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_resolve.hip')).read()
RS_BLOCK, RS_SPAN, RS_SPAN_FINE = (int(re.search(r'constexpr int %s = (\d+);' % name, _SOURCE).group(1)) for name in ('RS_BLOCK', 'RS_SPAN', 'RS_SPAN_FINE'))

pytestmark = pytest.mark.gpu


def fused(c, gpu, grads=True):
    from dirt_amd import shading
    return R.torch_form(c.image, c.add, c.go if grads else None, device=gpu, function=shading.resolve_image, **c.kw)


def check(got, c, name):
    worst = R.ratios(got, c.ref)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    wanted = {'out', 'd_image'} | ({'d_add'} if c.add is not None else set()) | ({'d_exposure'} if isinstance(c.kw['exposure'], np.ndarray) else set()) \
        | ({'d_white'} if isinstance(c.kw['white'], np.ndarray) else set())
    assert wanted <= set(worst), (wanted, set(worst))
    for kind, x in worst.items():
        assert got[kind].shape == np.shape(c.ref[kind]), (kind, got[kind].shape)
        assert x <= KERNEL * F32[kind], (name, kind, x)
    assert R.exact_where_massless(got, c.ref), name


def bits(x):
    return x.contiguous().view(torch.int32)


# ---- 1. the parity grid

@pytest.mark.parametrize('name', R.NAMES)
def test_the_kernels_against_the_restatement(gpu, name):
    check(fused(R.case(name), gpu), R.case(name), name)


# ---- 2. which gradients are wanted

def _operands(c, gpu, want=(True, True, True, True)):
    dev = lambda x, on: None if x is None else torch.tensor(x, device=gpu).requires_grad_(on)   # noqa: E731
    return [dev(c.image, want[0]), dev(c.add, want[1]), dev(c.kw['exposure'], want[2]), dev(c.kw['white'], want[3])]


def _call(c, operands):
    from dirt_amd import shading
    image, add, exposure, white = operands
    return shading.resolve_image(image, add=add, **dict(c.kw, exposure=exposure, white=white))


@pytest.mark.parametrize('want', list(itertools.product((False, True), repeat=4)), ids=lambda w: ''.join('x' if on else '-' for on in w))
def test_every_subset_of_wanted_gradients(gpu, want):
    """A gradient that is not wanted is not computed (a NULL pointer in the C call), and the others keep their bits"""
    c = R.case('grid-2-reinhard-srgb')
    go = torch.tensor(c.go, device=gpu)
    full = _operands(c, gpu)
    _call(c, full).backward(go)
    some = _operands(c, gpu, want)
    out = _call(c, some)
    assert out.requires_grad == any(want)
    if any(want):
        out.backward(go)
    for a, b, on in zip(full, some, want):
        assert (b.grad is not None) == on
        if on:
            assert torch.equal(bits(a.grad), bits(b.grad))


@pytest.mark.parametrize('want', [False, True])
def test_the_forward_saves_L_only_for_a_backward(gpu, want):
    from dirt_amd import _lib, lighting, shading
    c = R.case('grid-3-aces-srgb')
    image, add, exposure, _ = _operands(c, gpu, (False,) * 4)[:3] + [None]
    saved = []
    ctx = types.SimpleNamespace(needs_input_grad=(want, False, False, False, False), save_for_backward=lambda *t: saved.append(t))
    meta = (1, False, 17, 19, 3, 3, _lib.RESOLVE_CURVES['aces'], _lib.RESOLVE_ENCODINGS['srgb'], 0., 1., _lib.RESOLVE_CLAMP)
    shading._ResolveImage.forward(ctx, image, add, exposure[None], None, meta)
    linear = saved[0][0]
    if not want:
        assert linear is None
    else:
        form = lighting.resolve_image(image, add=add, factor=3, clamp=None)       # L itself: gain 1, no curve, no encoding, no clamp
        assert torch.equal(bits(linear), bits(form))


# ---- 3. shapes where the walk can go wrong

# (one output pixel and rows of 1, 2 and 3 floats modulo 4 -- every vector width and its tail -- are `resolve_reference.SMALL`,
# part of the parity grid above and of the F32 table)
SHAPES = [('span-%d-%d' % (S, W), dict(S=S, size=(3, W))) for S, span in ((1, RS_SPAN), (2, RS_SPAN), (3, RS_SPAN_FINE), (4, RS_SPAN_FINE))
       for W in (span - 1, span, span + 1)] \
    + [('many-workgroups', dict(S=1, size=(RS_BLOCK + 4, RS_SPAN + 4), curve='reinhard'))]     # more rows of partial sums than the reduction has lanes


@pytest.mark.parametrize('name, kw', SHAPES, ids=[n for n, _ in SHAPES])
def test_shapes_at_the_edges_of_the_walk(gpu, name, kw):
    """One workgroup's span, one pixel fewer and one more, for every S; more workgroups than `block_column_sum` has lanes"""
    c = R.Case(1000 + [n for n, _ in SHAPES].index(name), **dict(dict(curve=('aces', 'reinhard')[len(name) % 2]), **kw))
    if name == 'many-workgroups':
        assert c.ref['out'].shape[0] * -(-c.ref['out'].shape[1] // RS_SPAN) > RS_BLOCK
    check(fused(c, gpu), c, name)


# ---- 4. operands read in place

def _run(c, image, add, gpu):
    image, add = image.detach().requires_grad_(True), add.detach().requires_grad_(True)
    exposure, white = (torch.tensor(c.kw[k], device=gpu, requires_grad=True) for k in ('exposure', 'white'))
    out = _call(c, [image, add, exposure, white])
    grads = torch.autograd.grad(out, [image, add, exposure, white], torch.tensor(c.go, device=gpu))
    return [out.detach()] + list(grads)


@pytest.mark.parametrize('S', [1, 2, 3])
def test_operands_read_in_place_give_the_same_bits(gpu, S):
    """image = rgba[..., :3], add a slice of a 12-channel G-buffer, and both 4 bytes off a 16-byte boundary: the bits of the output
    and of every gradient are those of the call on contiguous copies"""
    c = R.Case(2000 + S, S=S, curve='reinhard', batch=2)
    image, add = torch.tensor(c.image, device=gpu), torch.tensor(c.add, device=gpu)
    want = _run(c, image, add, gpu)
    rgba = torch.cat([image, torch.full_like(image[..., :1], 7.)], -1)
    gbuffer = torch.cat([torch.full_like(image, -3.), torch.full_like(image[..., :2], 5.), add, torch.full_like(image, 9.), image[..., :1]], -1)
    assert gbuffer.shape[-1] == 12
    views = _run(c, rgba[..., :3], gbuffer[..., 5:8], gpu)

    def offset(x):      # the same values one float past a 16-byte boundary
        buffer = torch.empty(x.numel() + 1, device=gpu)
        y = buffer[1:].view(x.shape)
        y.copy_(x)
        assert y.data_ptr() % 16 == 4 and y.is_contiguous()
        return y

    shifted = _run(c, offset(image), offset(add), gpu)
    for a, b, d in zip(want, views, shifted):
        assert a.shape == b.shape == d.shape
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(d))
    assert want[1].data_ptr() != want[2].data_ptr()       # d add is a tensor of its own


# ---- 5. the paths that are exact

@pytest.mark.parametrize('S', [1, 2, 3, 4])
def test_the_linear_path_equals_the_torch_form_bit_for_bit(gpu, S):
    from dirt_amd import lighting
    c = R.case('grid-%d-linear-linear' % S)
    image, add, exposure = _operands(c, gpu, (False,) * 4)[:3]
    got = _call(c, [image, add, exposure, None])
    assert torch.equal(bits(got), bits(lighting.resolve_image(image, add=add, **dict(c.kw, exposure=exposure))))
    if S == 1:
        from dirt_amd import shading
        assert torch.equal(shading.resolve_image(image, add=add), (image + add).clamp(0., 1.))


# ---- 6. the same bits on every run

@pytest.mark.parametrize('name', ['batch-111', 'batch-010', 'grid-4-reinhard-srgb'])
def test_two_runs_give_the_same_bits(gpu, name):
    c = R.case(name)
    a, b = fused(c, gpu), fused(c, gpu)
    assert set(a) == {'out', 'd_image', 'd_add', 'd_exposure', 'd_white'}
    for kind in a:
        assert np.array_equal(a[kind].view(np.int32), b[kind].view(np.int32)), kind


def test_two_runs_of_many_workgroups_give_the_same_bits(gpu):
    c = R.Case(1100, S=1, size=(RS_BLOCK + 4, RS_SPAN + 4), curve='reinhard')
    a, b = fused(c, gpu), fused(c, gpu)
    for kind in a:
        assert np.array_equal(a[kind].view(np.int32), b[kind].view(np.int32)), kind


# ---- 7. values that are not finite

@pytest.mark.parametrize('curve', R.CURVES)
@pytest.mark.parametrize('encode', R.ENCODINGS)
@pytest.mark.parametrize('clamp', [(0., 1.), None])
def test_values_that_are_not_finite(gpu, curve, encode, clamp):
    """A NaN, a +inf and a -inf sample give what the torch form gives (the same bits, or a NaN in both), and every other pixel
    keeps the bits it has without them"""
    from dirt_amd import lighting, shading
    c = R.Case(3000, S=2, curve=curve, encode=encode, clamp=clamp)
    image, add, exposure, white = _operands(c, gpu, (False,) * 4)
    kw = dict(c.kw, exposure=exposure, white=white if curve == 'reinhard' else None)
    clean = shading.resolve_image(image, add=add, **kw)
    spots = {(2, 3, 0): float('nan'), (5, 7, 1): float('inf'), (9, 11, 2): float('-inf'), (12, 1, 0): float('inf')}
    for (r, col, ch), value in spots.items():
        image[2 * r + 1, 2 * col, ch] = value
    add[2 * 12, 2 * 1 + 1, 0] = float('-inf')     # inf + -inf
    got, form = shading.resolve_image(image, add=add, **kw), lighting.resolve_image(image, add=add, **kw)
    same = (bits(got) == bits(form)) | (torch.isnan(got) & torch.isnan(form))
    touched = torch.zeros_like(same)
    for r, col, ch in spots:
        touched[r, col, ch] = True
        assert same[r, col, ch], ((r, col, ch), float(got[r, col, ch]), float(form[r, col, ch]))
    assert torch.isnan(got[2, 3, 0]) and torch.isnan(got[12, 1, 0])
    assert torch.equal(bits(got)[~touched], bits(clean)[~touched])


# ---- 8. the C ABI, driven directly

GUARD = 12345.0


class Guarded:
    """A buffer of n floats between two runs of 64 guard values"""

    def __init__(self, n, gpu, values=None):
        self.n, self.all = n, torch.full((n + 128,), GUARD, device=gpu)
        if values is not None:
            self.inner.copy_(torch.as_tensor(values, device=gpu).reshape(-1))

    @property
    def inner(self):
        return self.all[64:64 + self.n]

    @property
    def ptr(self):
        return self.inner.data_ptr()

    def intact(self):
        return bool((self.all[:64] == GUARD).all() and (self.all[64 + self.n:] == GUARD).all())


def _abi_case():
    return R.Case(4000, S=2, curve='reinhard', batch=2, exposure_scene=True)


def _abi_call(c, gpu, skip=()):
    """Both entry points on guarded buffers -> (results, every guarded buffer)"""
    from dirt_amd import _lib
    lib = _lib.load()
    B, SH, SW, C = c.image.shape
    H, W, S = SH // 2, SW // 2, 2
    image, add, go = (torch.tensor(x, device=gpu) for x in (c.image, c.add, c.go))
    exposure, white = torch.tensor(c.kw['exposure'], device=gpu), torch.tensor(c.kw['white'], device=gpu).reshape(1)
    nbytes = lib.dirt_resolve_scratch_bytes(B, H, W, C, S)
    assert nbytes == 4 * B * H * -(-W // RS_SPAN) * (C + 1)
    out, lin = Guarded(B * H * W * C, gpu), Guarded(B * H * W * C, gpu)
    d = {'d_image': Guarded(image.numel(), gpu), 'd_add': Guarded(image.numel(), gpu), 'd_exposure': Guarded(B * C, gpu), 'd_white': Guarded(1, gpu)}
    scratch = Guarded(nbytes // 4, gpu)
    sizes = (B, H, W, C, S)
    tail = (B, 1, _lib.RESOLVE_CURVES['reinhard'], _lib.RESOLVE_ENCODINGS['srgb'], 0., 1., _lib.RESOLVE_CLAMP, None)
    _lib.check(lib.dirt_resolve_forward(image.data_ptr(), add.data_ptr(), exposure.data_ptr(), white.data_ptr(), out.ptr, lin.ptr, *sizes, C, C, B, B, *tail))
    at = lambda k: None if k in skip else d[k].ptr   # noqa: E731
    _lib.check(lib.dirt_resolve_backward(lin.ptr, exposure.data_ptr(), white.data_ptr(), go.data_ptr(), at('d_image'), at('d_add'), at('d_exposure'),
                                         at('d_white'), scratch.ptr, nbytes, *sizes, *tail))
    torch.cuda.synchronize()
    got = {'out': out.inner.cpu().numpy().reshape(B, H, W, C), 'd_image': d['d_image'].inner.cpu().numpy().reshape(c.image.shape),
           'd_add': d['d_add'].inner.cpu().numpy().reshape(c.image.shape), 'd_exposure': d['d_exposure'].inner.cpu().numpy().reshape(B, C),
           'd_white': d['d_white'].inner.cpu().numpy().reshape(())}
    return got, [out, lin, scratch] + list(d.values())


def test_the_c_abi_keeps_inside_its_buffers(gpu):
    c = _abi_case()
    got, buffers = _abi_call(c, gpu)
    assert all(b.intact() for b in buffers)
    check(got, c, 'abi')


@pytest.mark.parametrize('skip', [('d_image',), ('d_add', 'd_white'), ('d_exposure',), ('d_image', 'd_add')])
def test_the_c_abi_skips_null_gradients(gpu, skip):
    c = _abi_case()
    full, _ = _abi_call(c, gpu)
    got, buffers = _abi_call(c, gpu, skip)
    assert all(b.intact() for b in buffers)
    for kind in full:
        if kind in skip:
            assert (got[kind] == GUARD).all(), kind       # not written
        else:
            assert np.array_equal(got[kind].view(np.int32), full[kind].view(np.int32)), kind


def _refusal_calls(lib, gpu):
    x = torch.zeros(4096, device=gpu)
    p = x.data_ptr()
    fwd = dict(image=p, add=None, exposure=p, white=None, out=p, linear=None, scenes=1, rows=4, cols=5, channels=3, factor=2, image_stride=3, add_stride=3,
               image_scenes=1, add_scenes=1, exposure_scenes=1, white_scenes=1, curve=0, encode=0, lo=0., hi=1., flags=1)
    bwd = dict(linear=p, exposure=p, white=None, grad_out=p, grad_image=p, grad_add=None, grad_exposure=p, grad_white=None, scratch=p + 1024, scratch_bytes=4096,
               scenes=1, rows=4, cols=5, channels=3, factor=2, exposure_scenes=1, white_scenes=1, curve=0, encode=0, lo=0., hi=1., flags=1)
    forward = lambda **kw: lib.dirt_resolve_forward(*dict(fwd, **kw).values(), None)      # noqa: E731
    backward = lambda **kw: lib.dirt_resolve_backward(*dict(bwd, **kw).values(), None)    # noqa: E731
    need = lib.dirt_resolve_scratch_bytes(1, 4, 5, 3, 2)
    assert need == 4 * 4 * 4
    f, b = 'dirt_resolve_forward: ', 'dirt_resolve_backward: '
    return [
        (forward, dict(scenes=-1), f + '-1 scenes, 0..65535'),
        (forward, dict(scenes=65536), f + '65536 scenes, 0..65535'),
        (forward, dict(channels=0), f + '0 channels, 1..4'),
        (forward, dict(channels=5), f + '5 channels, 1..4'),
        (forward, dict(factor=0), f + 'factor=0, 1..4'),
        (backward, dict(factor=5), b + 'factor=5, 1..4'),
        (forward, dict(rows=-1), f + 'bad image size (rows=-1 cols=5), at most (2^31 - 1) / 4 each way and 2^36 pixels'),
        (forward, dict(cols=1 << 30), f + 'bad image size (rows=4 cols=1073741824), at most (2^31 - 1) / 4 each way and 2^36 pixels'),
        (backward, dict(rows=1 << 20, cols=1 << 20), b + 'bad image size (rows=1048576 cols=1048576), at most (2^31 - 1) / 4 each way and 2^36 pixels'),
        (forward, dict(curve=3), f + 'curve=3 is none of DIRT_RESOLVE_LINEAR, _REINHARD, _ACES'),
        (forward, dict(encode=2), f + 'encode=2 is neither DIRT_RESOLVE_ENCODE_LINEAR nor _SRGB'),
        (forward, dict(flags=2), f + 'unknown flags 0x2'),
        (forward, dict(lo=1., hi=0.), f + 'clamp bounds lo=1 > hi=0'),
        (backward, dict(lo=float('nan')), b + 'clamp bounds lo=nan > hi=1'),
        (forward, dict(exposure_scenes=2), f + 'exposure_scenes=2 is neither 1 nor scenes=1'),
        (forward, dict(curve=1), f + 'white goes with DIRT_RESOLVE_REINHARD and only with it (curve=1)'),
        (forward, dict(white=p), f + 'white goes with DIRT_RESOLVE_REINHARD and only with it (curve=0)'),
        (forward, dict(curve=1, white=p, white_scenes=3), f + 'white_scenes=3 is neither 1 nor scenes=1'),
        (forward, dict(image_stride=2), f + 'image_stride=2, a sample is 3 floats'),
        (forward, dict(add=p, add_stride=1), f + 'add_stride=1, a sample is 3 floats'),
        (forward, dict(image_scenes=2), f + 'image_scenes=2 is neither 1 nor scenes=1'),
        (forward, dict(add=p, add_scenes=0), f + 'add_scenes=0 is neither 1 nor scenes=1'),
        (forward, dict(image=None), f + 'image / exposure / out is NULL'),
        (backward, dict(grad_out=None), b + 'linear / exposure / grad_out is NULL'),
        (backward, dict(grad_white=p), b + 'grad_white without white'),
        (backward, dict(scratch=None), b + 'scratch is NULL or smaller than dirt_resolve_scratch_bytes (4096 < %d)' % need),
        (backward, dict(scratch_bytes=need - 4), b + 'scratch is NULL or smaller than dirt_resolve_scratch_bytes (%d < %d)' % (need - 4, need)),
        (backward, dict(scratch=p + 1026), b + 'scratch is not 4-byte aligned'),
    ]


def test_the_c_abi_refuses_with_a_sentence(gpu):
    """Every refusal with its full text from dirt_last_error, before any device work (the buffers are zeros and stay so)"""
    from dirt_amd import _lib
    lib = _lib.load()
    calls = _refusal_calls(lib, gpu)
    for function, change, text in calls:
        assert function(**change) == _lib.E_INVALID_ARGUMENT, change
        assert _lib.last_error() == text, change
    assert lib.dirt_resolve_scratch_bytes(-1, 4, 5, 3, 2) == 0 and lib.dirt_resolve_scratch_bytes(1, 4, 5, 5, 2) == 0
    assert lib.dirt_resolve_scratch_bytes(1, 4, 5, 3, 0) == 0
    # nothing to do: success, and the error is cleared
    assert calls[0][0](rows=0) == 0 and _lib.last_error() == ''
    assert calls[5][0](grad_image=None, grad_exposure=None) == 0 and _lib.last_error() == ''


def test_an_empty_call_launches_nothing(gpu):
    from dirt_amd import shading
    image = torch.zeros(2, 0, 8, 3, device=gpu, requires_grad=True)
    exposure = torch.ones(3, device=gpu, requires_grad=True)
    out = shading.resolve_image(image, factor=2, exposure=exposure, curve='aces', encode='srgb')
    assert out.shape == (2, 0, 4, 3)
    out.sum().backward()
    assert image.grad.shape == image.shape and torch.equal(exposure.grad, torch.zeros(3, device=gpu))


# ---- 9. captured in a graph

def test_a_captured_resolve_and_backward_replay_with_the_eager_bits(gpu):
    """The call and its backward make no host synchronisation: captured with torch.cuda.graph and replayed twice, the bits are
    the eager call's"""
    c = R.case('batch-111')
    operands = _operands(c, gpu, (False,) * 4)
    go = torch.tensor(c.go, device=gpu)

    def step():
        leaves = [x.detach().requires_grad_(True) for x in operands]
        out = _call(c, leaves)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, go))

    eager = [x.clone() for x in step()]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for x in captured:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(bits(a), bits(b))


# ---- 10. behind the rasteriser

def test_end_to_end_behind_rasterise(gpu):
    """Two triangles rasterised at 32 x 32, resolved to 16 x 16 with 'aces' and 'srgb': against the torch form on the same render,
    within KERNEL F32 of each element's mass off the kinks; the gradient reaches the vertex colours"""
    import dirt_amd as dirt
    from dirt_amd import lighting, shading
    vertices = torch.tensor([[-0.8, -0.7, 0.1, 1.], [0.9, -0.6, 0.2, 1.], [0.1, 0.8, 0.3, 1.], [-0.6, 0.7, 0.5, 1.], [0.7, 0.9, 0.4, 1.], [0.2, -0.9, 0.6, 1.]],
                            device=gpu)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=gpu)
    colors = torch.tensor([[0.9, 0.2, 0.1], [0.1, 3.0, 0.3], [0.2, 0.3, 6.0], [0.5, 0.5, 0.0], [1.5, 0.1, 0.9], [0.0, 0.02, 0.01]], device=gpu, requires_grad=True)
    background = torch.full((32, 32, 3), 0.05, device=gpu)
    exposure = torch.tensor([0.9, 1.2, 0.8], device=gpu)
    render = dirt.rasterise(background, vertices, colors, faces)
    got = shading.resolve_image(render, factor=2, exposure=exposure, curve='aces', encode='srgb')
    assert got.shape == (16, 16, 3)
    go = torch.tensor(np.random.default_rng(5).standard_normal((16, 16, 3)).astype(np.float32), device=gpu)
    ref = R.compose(render.detach().cpu().numpy(), factor=2, exposure=exposure.cpu().numpy(), curve='aces', encode='srgb', grad_out=go.cpu().numpy())
    go = go * torch.tensor(~ref['kink'], device=gpu)
    ref = R.compose(render.detach().cpu().numpy(), factor=2, exposure=exposure.cpu().numpy(), curve='aces', encode='srgb', grad_out=go.cpu().numpy())
    leaf = render.detach().requires_grad_(True)
    fused_out = shading.resolve_image(leaf, factor=2, exposure=exposure, curve='aces', encode='srgb')
    fused_out.backward(go)
    worst = R.ratios({'out': fused_out.detach().cpu().numpy(), 'd_image': leaf.grad.cpu().numpy()}, ref)
    form_leaf = render.detach().requires_grad_(True)
    form = lighting.resolve_image(form_leaf, factor=2, exposure=exposure, curve='aces', encode='srgb')
    form.backward(go)
    print(worst)
    assert worst['out'] <= KERNEL * F32['out'] and worst['d_image'] <= KERNEL * F32['d_image'], worst
    keep = torch.tensor(~ref['kink'], device=gpu)
    assert (got - form).abs()[keep].max() <= 1e-5
    covered = int((render.detach() != 0.05).any(-1).sum())
    assert covered >= 100
    got.backward(go)
    assert colors.grad is not None and (colors.grad.abs().sum(-1) > 0).all()
