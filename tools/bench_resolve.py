"""The fused last stage (dirt_amd.shading.resolve_image) against the route available before it, composed in torch: the two
radiance images added, `reshape(...).mean((1, 3))`, the torch form's exposure, ACES curve and sRGB encode
(`lighting.resolve_image` at factor 1 on the resolved image), the clamp.  Timed with HIP events after warm-up, in one process,
the two legs alternating (the method of tools/bench_shade.py), with `add`, three gains as a tensor, curve='aces', encode='srgb', at
      2048 x 2048 x 3 -> 1024 x 1024 x 3    factor 2
      1024 x 1024 x 3 -> 1024 x 1024 x 3    factor 1
      1280 x  960 x 3 ->  640 x  480 x 3    factor 2
Per shape:
      forward            the call alone, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to image, add and the gains.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  The bar: the fused
leg's slowest block under the composed leg's fastest, at each shape, forward and forward + backward;
`fused_slowest_under_composed_fastest` says whether it was.  Beside them `c_calls`: the three C entry points called directly
(forward without L, forward with L, backward with every gradient), their median time, the bytes each must move, computed from the
shapes, and those bytes over the time as a share of 8 TB/s.
usage (GPU box): python tools/bench_resolve.py [steps] [repeats]     (prints one JSON line, writes profiles/resolve.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from dirt_amd import _lib, lighting, shading  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

GAINS = (0.9, 1.2, 0.8)
SHAPES = ((1024, 1024, 2), (1024, 1024, 1), (480, 640, 2))     # the output's height and width, the factor


def composed(image, add, factor, gains):
    """the route a user had: add, box filter, develop, clamp"""
    total = image + add
    if factor > 1:
        rows, cols, channels = total.shape
        total = total.reshape(rows // factor, factor, cols // factor, factor, channels).mean((1, 3))
    return lighting.resolve_image(total, exposure=gains, curve='aces', encode='srgb', clamp=None).clamp(0., 1.)


def time_c_calls(image, add, gains, height, width, factor, steps, repeats):
    """the C entry points by themselves: -> {call: {'ms', 'bytes', 'share_of_8TBs'}}"""
    lib = _lib.load()
    dev = image.device
    pixels, samples = height * width * 3, image.numel()
    out, linear, d_out = (torch.rand(height, width, 3, device=dev) for _ in range(3))
    d_image, d_add, d_gains = torch.empty_like(image), torch.empty_like(image), torch.empty(3, device=dev)
    nbytes = lib.dirt_resolve_scratch_bytes(1, height, width, 3, factor)
    scratch = torch.empty(nbytes // 4, device=dev)
    tail = (1, 1, _lib.RESOLVE_CURVES['aces'], _lib.RESOLVE_ENCODINGS['srgb'], 0., 1., _lib.RESOLVE_CLAMP, None)
    sizes = (1, height, width, 3, factor)

    def forward(lin):
        _lib.check(lib.dirt_resolve_forward(image.data_ptr(), add.data_ptr(), gains.data_ptr(), None, out.data_ptr(), lin, *sizes, 3, 3, 1, 1, *tail))

    def backward():
        _lib.check(lib.dirt_resolve_backward(linear.data_ptr(), gains.data_ptr(), None, d_out.data_ptr(), d_image.data_ptr(), d_add.data_ptr(),
                                             d_gains.data_ptr(), None, scratch.data_ptr(), nbytes, *sizes, *tail))

    calls = {'forward': (lambda: forward(None), 4 * (2 * samples + pixels)), 'forward_with_L': (lambda: forward(linear.data_ptr()), 4 * (2 * samples + 2 * pixels)),
             'backward': (backward, 4 * (2 * pixels + 2 * samples))}
    result = {}
    for name, (fn, moved) in calls.items():
        for _ in range(steps):
            fn()
        times = []
        for _ in range(repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) / steps)
        ms = sorted(times)[len(times) // 2]
        result[name] = {'ms': ms, 'min': min(times), 'max': max(times), 'bytes': moved, 'share_of_8TBs': moved / (ms * 1e-3) / 8e12}
    return result


def main():
    dev = torch.device('cuda', 0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    torch.manual_seed(0)
    out = {'steps': steps, 'repeats': repeats}
    for height, width, factor in SHAPES:
        image = (3. * torch.rand(factor * height, factor * width, 3, device=dev)).requires_grad_(True)
        add = torch.rand(factor * height, factor * width, 3, device=dev).requires_grad_(True)
        gains = torch.tensor(GAINS, device=dev).requires_grad_(True)
        d_out = torch.randn(height, width, 3, device=dev)
        shape = {}

        def fused_call():
            return shading.resolve_image(image, add=add, factor=factor, exposure=gains, curve='aces', encode='srgb')

        def composed_call():
            return composed(image, add, factor, gains)

        for name in ('forward', 'forward_backward'):
            def leg(fn, name=name):
                def step():
                    if name == 'forward':
                        with torch.no_grad():
                            fn()
                        return
                    image.grad = add.grad = gains.grad = None
                    fn().backward(d_out)
                return step

            t = time_alternating({'composed': leg(composed_call), 'fused': leg(fused_call)}, steps, repeats)
            t['speedup'] = t['composed']['ms'] / t['fused']['ms']
            t['fused_slowest_under_composed_fastest'] = t['fused']['max'] < t['composed']['min']
            shape[name] = t
        shape['c_calls'] = time_c_calls(image.detach(), add.detach(), gains.detach(), height, width, factor, steps, repeats)
        out['%dx%dx3_to_%dx%dx3' % (factor * height, factor * width, height, width)] = shape
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'resolve.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps; c_calls: the C entry '
                           'points alone, bytes from the shapes (tools/bench_resolve.py)' % (repeats, steps), 'bench_resolve': out}, fh, indent=1)


if __name__ == '__main__':
    main()
