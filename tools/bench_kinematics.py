#!/usr/bin/env python3
"""Times `dirt_amd.kinematics.pose_skeleton` beside the torch loop users write for the forward kinematics of a skeleton --
per joint one matrices.rodrigues, two matrices.translation and up to three compose, every joint after its parent
(examples/fit_pose_fused.py's bone_transforms, for a tree) -- forward and forward + backward to both inputs, with HIP
events, the two paths in alternation on the same GPU.  Writes profiles/kinematics.json; DESIGN.md §7e has the table.

    python tools/bench_kinematics.py [--reps 200] [--out profiles/kinematics.json]
    python tools/bench_kinematics.py --trace      # a short fused-only loop for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/bench_kinematics.py --step       # the share of the torch loop in a step of examples/fit_body_pose_fused.py

Per configuration and path: `reps` timed calls in alternating blocks of 50 after 20 untimed ones, each call between two
events on the current stream (so a figure includes the launch gaps between the path's kernels, which is what a fitting
loop pays); reported are the median and the minimum in microseconds, and beside them the device operations per forward +
backward call as torch.profiler counts them.  DIRT_AMD_LIBRARY selects another build of the library (the one-wave
workgroup for small rigs against four waves: `python -m dirt_amd.build --out ... --flags -DDIRT_KINEMATICS_SMALL_BLOCK=256`).
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dirt_amd import kinematics, matrices  # noqa: E402

SMPL = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def random_tree(rng, J):
    return [-1] + rng.integers(0, np.arange(1, J)).tolist()


def smplx_like(rng):
    """55 joints: the SMPL body's first 22, then jaw and eyes on the head and fifteen finger joints (five chains of three) per wrist"""
    parents = list(SMPL[:22]) + [15, 15, 15]
    for wrist in (20, 21):
        for _ in range(5):
            parents += [wrist, len(parents), len(parents) + 1]
    return parents


# (name, parents, B)
def configurations(rng):
    return (('smpl', list(SMPL), 1), ('smpl', list(SMPL), 32), ('smplx', smplx_like(rng), 32), ('tree256', random_tree(rng, 256), 8),
            ('chain64', list(range(-1, 63)), 1))


def torch_loop(rotations, joints, parents):
    """the composition as users write it: -> (transforms [.., J, 4, 4], posed_joints [.., J, 3])"""
    out = []
    for j, q in enumerate(parents):
        pivot = joints[..., j, :]
        local = matrices.compose(matrices.translation(-pivot), matrices.rodrigues(rotations[..., j, :]), matrices.translation(pivot))
        out.append(local if q < 0 else matrices.compose(local, out[q]))
    T = torch.stack(out, -3)
    p4 = torch.cat([joints, torch.ones_like(joints[..., :1])], -1)
    return T, (p4[..., None, :] @ T)[..., 0, :3]


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


def alternate(fns, reps, block=50):
    """{name: figures in microseconds}: the paths timed in alternating blocks of `block` calls"""
    times = {k: [] for k in fns}
    for _ in range(max(reps // block, 1)):
        for k, fn in fns.items():
            times[k] += timed(fn, block)
    return {k: {'median_us': round(float(np.median(t)), 2), 'min_us': round(float(np.min(t)), 2), 'n': len(t)} for k, t in times.items()}


def launches(run, steps=5):
    """device operations (kernels and copies) per forward + backward call of `run`, counted by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    run(True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            run(True)
        torch.cuda.synchronize()
    return round(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA) / steps, 1)


def runner(stage, r0, p0, gT, gq):
    def run(backward):
        r, p = r0.detach().requires_grad_(backward), p0.detach().requires_grad_(backward)
        T, q = stage(r, p)
        if backward:
            torch.autograd.backward([T, q], [gT, gq])
    return run


def step_share(args):
    """A step of examples/fit_body_pose_fused.py with the kernel and with the torch loop in its place: what share of a whole
    pose-fitting step the loop is."""
    spec = importlib.util.spec_from_file_location('fit_body_pose_fused', os.path.join(ROOT, 'examples', 'fit_body_pose_fused.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    from dirt_amd import geometry, skinning
    dev = torch.device('cuda', 0)
    rest, faces, bone_indices, bone_weights, joints = ex.build_figure(dev)
    topology, skin = geometry.MeshTopology(faces, rest.shape[0]), skinning.SkinWeights(bone_indices, bone_weights, len(ex.FIGURE))
    skeleton = kinematics.Skeleton(ex.PARENTS, device=dev)
    vp = matrices.translation(torch.tensor([0., 0., -2.5], device=dev)) @ \
        matrices.perspective_projection(near=0.1, far=20., right=0.06, aspect=float(ex.frame_height) / ex.frame_width).to(dev)
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.3, -1.], device=dev), dim=0)
    r0 = 0.3 * torch.randn(len(ex.FIGURE), 3, device=dev, generator=torch.Generator(dev).manual_seed(0))
    fused = kinematics.pose_skeleton
    with torch.no_grad():
        target_image, target_points = ex.render(rest, skin, topology, skeleton, joints, r0 + 0.1, vp, light)

    def step(which):
        def run():
            kinematics.pose_skeleton = fused if which == 'fused' else (lambda r, p, s: torch_loop(r, p, ex.PARENTS))
            try:
                r = r0.detach().requires_grad_(True)
                image, points = ex.render(rest, skin, topology, skeleton, joints, r, vp, light)
                loss = ((image - target_image) ** 2).mean() + ex.KEY_POINT_WEIGHT * ((points - target_points) ** 2).mean()
                torch.autograd.grad(loss, r)
            finally:
                kinematics.pose_skeleton = fused
        return run

    def kin_only(which):
        stage = (lambda r, p: fused(r, p, skeleton)) if which == 'fused' else (lambda r, p: torch_loop(r, p, ex.PARENTS))
        run = runner(stage, r0, joints, torch.randn(len(ex.FIGURE), 4, 4, device=dev), torch.randn(len(ex.FIGURE), 3, device=dev))
        return lambda: run(True)

    row = {'example': 'fit_body_pose_fused', 'J': len(ex.FIGURE), 'V': int(rest.shape[0]), 'frame': [ex.frame_width, ex.frame_height]}
    row.update(alternate({'step_fused': step('fused'), 'step_torch_loop': step('torch_loop'),
                          'kinematics_fused_forward_backward': kin_only('fused'), 'kinematics_torch_loop_forward_backward': kin_only('torch_loop')}, args.reps))
    row['torch_loop_share_of_its_step'] = round(row['kinematics_torch_loop_forward_backward']['median_us'] / row['step_torch_loop']['median_us'], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kinematics.json'))
    ap.add_argument('--trace', action='store_true', help='run 20 fused forward + backward steps per configuration and exit (for a kernel trace)')
    ap.add_argument('--step', action='store_true', help='time a whole step of examples/fit_body_pose_fused.py with either path and exit')
    ap.add_argument('--fused-only', action='store_true', help='time the fused path alone (A/B builds of the library)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    if args.step:
        row = step_share(args)
        print(json.dumps(row), flush=True)
        with open(args.out, 'w') as fh:
            json.dump(row, fh, indent=1)
            fh.write('\n')
        return
    rng = np.random.default_rng(0)
    results = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'library': os.environ.get('DIRT_AMD_LIBRARY', 'default'), 'configurations': []}
    for name, parents, B in configurations(rng):
        J = len(parents)
        lead = (B,) if B > 1 else ()
        axes = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal(lead + (J, 3)).astype(np.float32)), dim=-1)
        r0 = (axes * torch.from_numpy(rng.uniform(0.3, 3.0, lead + (J, 1)).astype(np.float32))).to(dev)
        p0 = torch.from_numpy(rng.uniform(-1., 1., (J, 3)).astype(np.float32)).to(dev)      # one body shape for every scene
        gT, gq = torch.randn(lead + (J, 4, 4), device=dev), torch.randn(lead + (J, 3), device=dev)
        skeleton = kinematics.Skeleton(parents, device=dev)
        paths = {'fused': runner(lambda r, p: kinematics.pose_skeleton(r, p, skeleton), r0, p0, gT, gq)}
        if not args.fused_only:
            paths['torch_loop'] = runner(lambda r, p: torch_loop(r, p, parents), r0, p0, gT, gq)
        if args.trace:
            for _ in range(20):
                paths['fused'](True)
            torch.cuda.synchronize()
            continue
        row = {'skeleton': name, 'J': J, 'B': B, 'levels': skeleton.num_levels}
        fns = {}
        for path, run in paths.items():
            fns[path + '_forward'] = (lambda run=run: run(False))
            fns[path + '_forward_backward'] = (lambda run=run: run(True))
        row.update(alternate(fns, args.reps))
        row['launches_forward_backward'] = {path: launches(run) for path, run in paths.items()}
        results['configurations'].append(row)
        print(json.dumps(row), flush=True)
    if args.trace:
        return
    with open(args.out, 'w') as fh:
        json.dump(results, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
