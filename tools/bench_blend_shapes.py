#!/usr/bin/env python3
"""Times `dirt_amd.blendshapes.blend_shapes` beside the torch composition users write for a blend-shape model -- SMPL's form:
the first Ks directions shape the mesh, a dense-regressor einsum takes the joints from it, the remaining directions (pose
correctives) are added after -- forward and forward + backward (to the coefficients and, with per-scene templates, to the
template; gradients arrive from both outputs), with HIP events, the paths in alternation on the same GPU.  Writes
profiles/blend_shapes.json; DESIGN.md §7f has the table.

    python tools/bench_blend_shapes.py [--reps 200] [--out profiles/blend_shapes.json]
    python tools/bench_blend_shapes.py --trace       # a short fused-only loop for `rocprofv3 --kernel-trace --stats -- ...`

Per configuration and path: `reps` timed calls after 20 untimed ones, each call between two events on the current stream
(so a figure includes the launch gaps between the path's kernels, which is what a fitting loop pays); reported are the
median and the minimum in microseconds, and beside them the device operations per forward + backward call as
torch.profiler counts them.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dirt_amd import blendshapes  # noqa: E402

# (V, K, Ks, J, B, per-scene templates): an SMPL-sized body (10 shape + 207 pose-corrective directions) for one scene and 32, the
# same with per-scene templates, a 75 000-vertex scan with 64 directions, and the shape directions alone
CONFIGURATIONS = ((6890, 217, 10, 24, 1, False), (6890, 217, 10, 24, 32, False), (6890, 217, 10, 24, 32, True),
                  (75000, 64, 64, 64, 1, False), (75000, 64, 64, 64, 8, False), (6890, 10, 10, 24, 32, False))


def make_inputs(rng, V, K, J, B, dev):
    """template [V, 3], directions [K, V, 3], a regressor [J, V] of twelve non-zeros per joint, coefficients [B, K]"""
    reg = np.zeros((J, V), np.float32)
    for j in range(J):
        w = rng.uniform(0.05, 1., 12)
        reg[j, rng.permutation(V)[:12]] = w / w.sum()
    return (torch.from_numpy(rng.uniform(-1., 1., (V, 3)).astype(np.float32)).to(dev),
            torch.from_numpy((0.1 * rng.standard_normal((K, V, 3))).astype(np.float32)).to(dev), torch.from_numpy(reg).to(dev),
            torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).to(dev))


def torch_composition(template, c, table, regressor, Ks):
    """what a user writes: template + c @ D.reshape(K, -1), the joints by a dense-regressor einsum from the shaped mesh"""
    B, V = c.shape[0], regressor.shape[1]
    shaped = template + (c[:, :Ks] @ table[:Ks]).reshape(B, V, 3)
    joints = torch.einsum('jv,bvc->bjc', regressor, shaped)
    return (shaped + (c[:, Ks:] @ table[Ks:]).reshape(B, V, 3) if Ks < table.shape[0] else shaped), joints


def timed(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def alternate(fns, reps, rounds=4):
    """{name: [microseconds]}: the paths timed in `rounds` alternating blocks"""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k] += timed(fn, reps // rounds)
    return {k: {'median_us': round(float(np.median(t)), 2), 'min_us': round(float(np.min(t)), 2), 'n': len(t)} for k, t in times.items()}


def launches(run, steps=10):
    """device operations (kernels and copies) per forward + backward call of `run`, counted by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    run(True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            run(True)
        torch.cuda.synchronize()
    return round(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA) / steps, 1)


def runner(stage, t0, c0, grads, grad_template):
    def run(backward):
        t = t0.detach().requires_grad_(backward and grad_template)
        c = c0.detach().requires_grad_(backward)
        outs = stage(t, c)
        if backward:
            torch.autograd.backward(outs, grads)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'blend_shapes.json'))
    ap.add_argument('--trace', action='store_true', help='run 20 fused forward + backward steps per configuration and exit (for a kernel trace)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    results = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'configurations': []}
    for V, K, Ks, J, B, per_scene in CONFIGURATIONS:
        template, directions, regressor, c0 = make_inputs(rng, V, K, J, B, dev)
        shapes = blendshapes.BlendShapes(directions, regressor, Ks)
        table = directions.reshape(K, 3 * V)
        t0 = template[None].repeat(B, 1, 1).contiguous() if per_scene else template
        grads = [torch.randn(B, V, 3, device=dev), torch.randn(B, J, 3, device=dev)]
        paths = {'fused': runner(lambda t, c: blendshapes.blend_shapes(t, c, shapes), t0, c0, grads, per_scene),
                 'torch': runner(lambda t, c: torch_composition(t, c, table, regressor, Ks), t0, c0, grads, per_scene)}
        if args.trace:
            for _ in range(20):
                paths['fused'](True)
            torch.cuda.synchronize()
            continue
        row = {'V': V, 'K': K, 'Ks': Ks, 'J': J, 'B': B, 'template': 'per scene' if per_scene else 'shared', 'table_MB': round(shapes.packed.numel() * 4 / 1e6, 1)}
        fns = {}
        for name, run in paths.items():
            fns[name + '_forward'] = (lambda run=run: run(False))
            fns[name + '_forward_backward'] = (lambda run=run: run(True))
        row.update(alternate(fns, args.reps))
        row['launches_forward_backward'] = {name: launches(run) for name, run in paths.items()}
        results['configurations'].append(row)
        print(json.dumps(row), flush=True)
    if args.trace:
        return
    with open(args.out, 'w') as fh:
        json.dump(results, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
