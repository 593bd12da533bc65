#!/usr/bin/env python3
"""Times `dirt_amd.skinning.skin_vertices` beside the two torch compositions users write for linear-blend skinning -- the
gather form ([B, V, K, 4, 4] gathered and reduced) and the dense form ([V, J] @ [J, 16]) -- forward and forward +
backward (to the bone transforms and, with per-scene vertices, to the vertices), with HIP events, the paths in
alternation on the same GPU.  Writes profiles/skinning.json; DESIGN.md §7d has the table.

    python tools/bench_skinning.py [--reps 200] [--out profiles/skinning.json]
    python tools/bench_skinning.py --trace       # a short fused-only loop for `rocprofv3 --kernel-trace --stats -- ...`

Per configuration and path: `reps` timed calls after 20 untimed ones, each call between two events on the current stream
(so a figure includes the launch gaps between the path's kernels, which is what a fitting loop pays); reported are the
median and the minimum in microseconds, and beside them the device operations per forward + backward call as
torch.profiler counts them.  The last block times the fused forward + backward for several chunk sizes of the
inverted index (every vertex on bone 0: the root of a skeleton).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dirt_amd import skinning  # noqa: E402

# (V, J, K, B, per-scene vertices): an SMPL-sized body, one pose and 32 poses of a shared rest mesh; a 75 000-vertex scan
CONFIGURATIONS = ((6890, 24, 4, 1, False), (6890, 24, 4, 32, False), (75000, 64, 4, 1, False), (75000, 64, 4, 8, False))
# beside them: per-scene vertices, and the two bone counts either side of the LDS-staging limit (256 staged, 257 not)
EXTRA = ((6890, 24, 4, 32, True), (6890, 256, 4, 32, False), (6890, 257, 4, 32, False))
CHUNKS = (256, 512, 1024, 2048, 4096)


def make_inputs(rng, V, J, K, B, dev):
    """rest vertices [V, 3], (indices, weights) [V, K] with slot 0 on bone 0 (the root names every vertex), transforms
    [B, J, 4, 4] (or [J, 4, 4] for B = 1)"""
    idx = rng.integers(0, J, (V, K)).astype(np.int32)
    idx[:, 0] = 0
    w = rng.uniform(0.05, 1., (V, K))
    T = np.tile(np.eye(4), (B, J, 1, 1)) + rng.uniform(-0.1, 0.1, (B, J, 4, 4))
    return (torch.from_numpy(rng.uniform(-1., 1., (V, 3)).astype(np.float32)).to(dev), torch.from_numpy(idx).to(dev),
            torch.from_numpy((w / w.sum(1, keepdims=True)).astype(np.float32)).to(dev),
            torch.from_numpy((T if B > 1 else T[0]).astype(np.float32)).to(dev))


def torch_gather(v, idx, w, T):
    """the gather form: [.., V, K, 4, 4] gathered, weighted and summed over K, then the per-vertex product"""
    v4 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
    M = (w[:, :, None, None] * T[..., idx, :, :]).sum(-3)
    return (v4[..., None, :] @ M)[..., 0, :3]


def torch_dense(v, dense, T):
    """the dense form: [V, J] @ [J, 16] materialises [.., V, 4, 4]"""
    v4 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
    M = (dense @ T.reshape(T.shape[:-2] + (16,))).reshape(T.shape[:-3] + (-1, 4, 4))
    return (v4[..., None, :] @ M)[..., 0, :3]


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


def runner(stage, v0, T0, go, grad_vertices):
    def run(backward):
        v = v0.detach().requires_grad_(backward and grad_vertices)
        T = T0.detach().requires_grad_(backward)
        out = stage(v, T)
        if backward:
            out.backward(go)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'skinning.json'))
    ap.add_argument('--trace', action='store_true', help='run 20 fused forward + backward steps per configuration and exit (for a kernel trace)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    results = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'chunk': skinning.CHUNK, 'configurations': [], 'chunks': []}
    for V, J, K, B, per_scene in CONFIGURATIONS + EXTRA:
        rest, idx, w, T0 = make_inputs(rng, V, J, K, B, dev)
        skin = skinning.SkinWeights(idx, w, J)
        dense = skin.dense()
        v0 = rest[None].repeat(B, 1, 1).contiguous() if per_scene else rest
        go = torch.randn(((B,) if B > 1 else ()) + (V, 3), device=dev)
        idx64 = idx.long()
        paths = {'fused': runner(lambda v, T: skinning.skin_vertices(v, skin, T), v0, T0, go, per_scene),
                 'torch_gather': runner(lambda v, T: torch_gather(v, idx64, w, T), v0, T0, go, per_scene),
                 'torch_dense': runner(lambda v, T: torch_dense(v, dense, T), v0, T0, go, per_scene)}
        if args.trace:
            for _ in range(20):
                paths['fused'](True)
            torch.cuda.synchronize()
            continue
        row = {'V': V, 'J': J, 'K': K, 'B': B, 'vertices': 'per scene' if per_scene else 'shared rest mesh', 'chunks': skin.num_chunks}
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
    for V, J, K, B, _ in CONFIGURATIONS:
        rest, idx, w, T0 = make_inputs(rng, V, J, K, B, dev)
        go = torch.randn(((B,) if B > 1 else ()) + (V, 3), device=dev)
        fns = {}
        for chunk in CHUNKS:
            skin = skinning.SkinWeights(idx, w, J, chunk=chunk)
            fns['chunk=%d' % chunk] = (lambda run=runner(lambda v, T, skin=skin: skinning.skin_vertices(v, skin, T), rest, T0, go, False): run(True))
        row = {'V': V, 'J': J, 'K': K, 'B': B}
        row.update(alternate(fns, args.reps))
        results['chunks'].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, 'w') as fh:
        json.dump(results, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
