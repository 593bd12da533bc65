#!/usr/bin/env python3
"""Times `dirt_amd.geometry.vertex_stage` beside the torch composition it replaces (`lighting.vertex_normals` plus the two
matmuls), forward and forward + backward, with HIP events, the two in alternation on the same GPU.  Writes
profiles/geometry.json; DESIGN.md §7c has the table.

    python tools/bench_geometry.py [--reps 200] [--out profiles/geometry.json]

Per configuration and path: `reps` timed calls after 20 untimed ones, each call between two events on the current stream
(so a figure includes the launch gaps between the path's kernels, which is what a fitting loop pays); reported are the
median and the minimum in microseconds.  The last block times the forward on a fan (one vertex in 2000 faces) and on the
75 000-vertex grid for several values of the long-list threshold.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dirt_amd import geometry, lighting, matrices  # noqa: E402


def grid(rng, num_vertices):
    """a jittered square grid of exactly `num_vertices` shared vertices and its two triangles per cell (F ~ 2 V)"""
    cols = int(np.ceil(np.sqrt(num_vertices)))
    idx = np.arange(num_vertices)
    h = 2. / cols
    v = np.concatenate([np.stack([idx % cols, idx // cols], 1) * h - 1. + rng.uniform(-0.2, 0.2, (num_vertices, 2)) * h,
                        rng.uniform(-0.3, 0.3, (num_vertices, 1)) * h], 1).astype(np.float32)
    a = idx[(idx % cols < cols - 1) & (idx + cols + 1 < num_vertices)]
    return v, np.concatenate([np.stack([a, a + 1, a + cols + 1], 1), np.stack([a, a + cols + 1, a + cols], 1)]).astype(np.int32)


def fan(rng, blades=2000):
    theta, r = rng.uniform(0., 2. * np.pi, blades), rng.uniform(0.6, 1., (blades, 2))
    rim = np.stack([np.stack([r[:, k] * np.cos(theta + 0.9 * k), r[:, k] * np.sin(theta + 0.9 * k), rng.uniform(-0.1, 0.1, blades)], 1) for k in (0, 1)], 1)
    b = np.arange(blades)
    return (np.concatenate([np.zeros((1, 3)), rim.reshape(-1, 3)]).astype(np.float32),
            np.stack([np.zeros_like(b), 1 + 2 * b, 2 + 2 * b], 1).astype(np.int32))


def torch_stage(v, faces, model, vp, pre_split):
    v4 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
    world = v4 @ model
    normals = (lighting.vertex_normals_pre_split if pre_split else lighting.vertex_normals)(world, faces)
    return world @ vp, world, normals


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'geometry.json'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    model = matrices.rodrigues(torch.tensor([0., 0.5, 0.], device=dev))
    vp = matrices.translation(torch.tensor([0., 0., -3.], device=dev)) @ matrices.perspective_projection(0.1, 20., 0.1, 0.75).to(dev)
    meshes = {'shared V=5000': grid(rng, 5000) + (False,), 'shared V=75000': grid(rng, 75000) + (False,)}
    v, f = grid(rng, 5200)
    f = f[:10000]
    assert len(f) == 10000
    meshes['split V=30000 (pre_split)'] = (v[f.reshape(-1)], np.arange(30000, dtype=np.int32).reshape(-1, 3), True)
    results = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'configurations': [], 'long_list': []}
    for name, (v_np, f_np, pre_split) in meshes.items():
        for batch in (1, 8):
            v0 = torch.from_numpy(np.repeat(v_np[None], batch, 0).copy()).to(dev)
            faces = torch.from_numpy(f_np).to(dev)
            topology = geometry.MeshTopology(faces, v_np.shape[0])
            go = [torch.randn(batch, v_np.shape[0], c, device=dev) for c in (4, 4, 3)]

            def run(stage, backward):
                v = v0.detach().requires_grad_(backward)
                outs = stage(v)
                if backward:
                    torch.autograd.backward(outs, go)

            fused = lambda v: geometry.vertex_stage(v, topology, model, vp, pre_split=pre_split)   # noqa: E731
            composed = lambda v: torch_stage(v, faces, model, vp, pre_split)                         # noqa: E731
            row = {'mesh': name, 'V': int(v_np.shape[0]), 'F': int(f_np.shape[0]), 'B': batch}
            row.update(alternate({'fused_forward': lambda: run(fused, False), 'torch_forward': lambda: run(composed, False),
                                  'fused_forward_backward': lambda: run(fused, True), 'torch_forward_backward': lambda: run(composed, True)}, args.reps))
            results['configurations'].append(row)
            print(json.dumps(row), flush=True)
    for name, (v_np, f_np) in (('fan, hub in 2000 faces', fan(rng)), ('shared V=75000', grid(rng, 75000))):
        v0 = torch.from_numpy(v_np).to(dev)
        topology = geometry.MeshTopology(torch.from_numpy(f_np).to(dev), v_np.shape[0])
        row = {'mesh': name}
        for threshold in (16, 64, 256, 65535):
            geometry.LONG_LIST = threshold
            try:
                t = timed(lambda: geometry.vertex_stage(v0, topology, model, vp), args.reps)
            finally:
                geometry.LONG_LIST = None
            row['long_list=%d' % threshold] = {'median_us': round(float(np.median(t)), 2), 'min_us': round(float(np.min(t)), 2)}
        results['long_list'].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, 'w') as fh:
        json.dump(results, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
