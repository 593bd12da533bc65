"""GPU box: tangent-space normal mapping (dirt_tangent.hip, dirt_normal_map.hip) -- HIP-event times of
`geometry.vertex_tangents` on a grid mesh of about 10 000 faces and of `shading.perturb_normals` on a 1024 x 1024 G-buffer of 12
channels (normal map read in place from channels 5:8 of an 8-channel look-up), forward and backward, and beside them, in the same
process on the same inputs, their torch forms: `lighting.vertex_tangents`, and `lighting.perturb_normals` on slices plus the
`torch.cat` back into the G-buffer.  Every figure is the mean of `n` calls between two events after 5 warm-up calls, through the
public API (so a backward is one torch.autograd.grad over a retained graph: the kernels plus the autograd node's allocations);
the C ABI calls alone are timed too, with the bytes each pixel kernel has to move.
usage: python tools/bench_normal_map.py [json path, default profiles/normal_map.json] [--pixels 1024] [--grid 72]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import _lib, geometry, lighting, rasterise_ops as _ops, shading  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
out_path = next((a for a in argv if a.endswith('.json')), os.path.join(ROOT, 'profiles', 'normal_map.json'))
P = int(argv[argv.index('--pixels') + 1]) if '--pixels' in argv else 1024
GRID = int(argv[argv.index('--grid') + 1]) if '--grid' in argv else 72
CG, ON, OT = 12, 3, 8
if not torch.cuda.is_available():
    sys.exit('bench_normal_map.py measures on an MI355X; no GPU found')
dev = torch.device('cuda:0')
lib = _lib.load()
stream = _ops._stream_handle(dev)


def timed(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us


def forward_backward(make_out, leaves, g):
    """-> (forward us, backward us) of out = make_out() and torch.autograd.grad(out, leaves, g)"""
    out = make_out()
    return timed(make_out), timed(lambda: torch.autograd.grad(out, leaves, g, retain_graph=True))


rng = np.random.default_rng(0)

# ---- the mesh: a GRID x GRID sheet with a height field, uv = a rotated copy of (x, y)
ys, xs = np.meshgrid(np.linspace(-1., 1., GRID), np.linspace(-1., 1., GRID), indexing='ij')
position = np.stack([xs, ys, 0.2 * np.sin(3. * xs) * np.cos(2. * ys)], -1).reshape(-1, 3).astype(np.float32)
index = np.arange(GRID * GRID).reshape(GRID, GRID)
quads = np.stack([index[:-1, :-1], index[:-1, 1:], index[1:, 1:], index[1:, :-1]], -1).reshape(-1, 4)
faces_np = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]]).astype(np.int32)
uv_np = (position[:, :2] @ np.array([[0.8, 0.6], [-0.6, 0.8]], np.float32) * 0.4 + 0.5).astype(np.float32)
vertices = torch.from_numpy(position).to(dev).requires_grad_(True)
faces, uvs = torch.from_numpy(faces_np).to(dev), torch.from_numpy(uv_np).to(dev)
topology = geometry.MeshTopology(faces, GRID * GRID)
normals = lighting.vertex_normals(vertices.detach(), faces).requires_grad_(True)
g_t = torch.from_numpy(rng.standard_normal((GRID * GRID, 4)).astype(np.float32)).to(dev)

# ---- the G-buffer: unit normals, tangents a quarter turn off them, handedness +-1; the map in an 8-channel look-up
n_px = rng.standard_normal((P, P, 3))
n_px /= np.linalg.norm(n_px, axis=-1, keepdims=True)
t_px = np.cross(n_px, rng.standard_normal((P, P, 3)))
gbuf = rng.standard_normal((P, P, CG)).astype(np.float32)
gbuf[..., ON:ON + 3], gbuf[..., OT:OT + 3], gbuf[..., OT + 3] = n_px, t_px, np.where(rng.uniform(size=(P, P)) < 0.5, -1., 1.)
gb = torch.from_numpy(gbuf).to(dev).requires_grad_(True)
looked_up = torch.from_numpy(rng.uniform(0., 1., (P, P, 8)).astype(np.float32)).to(dev).requires_grad_(True)
g_g = torch.from_numpy(rng.standard_normal((P, P, CG)).astype(np.float32)).to(dev)


def torch_route():
    bumped = lighting.perturb_normals(gb[..., ON:ON + 3], gb[..., OT:OT + 4], looked_up[..., 5:8])
    return torch.cat([gb[..., :ON], bumped, gb[..., ON + 3:]], dim=-1)


results = {
    'vertex_tangents': forward_backward(lambda: geometry.vertex_tangents(vertices, normals, uvs, topology), [vertices, normals], g_t),
    'vertex_tangents_torch': forward_backward(lambda: lighting.vertex_tangents(vertices, normals, uvs, faces), [vertices, normals], g_t),
    'perturb_normals': forward_backward(lambda: shading.perturb_normals(gb, looked_up[..., 5:8], normals=ON, tangents=OT), [gb, looked_up], g_g),
    'perturb_normals_torch_cat': forward_backward(torch_route, [gb, looked_up], g_g),
}

# the C ABI calls alone: no allocation, no autograd node
with torch.no_grad():
    V, F = GRID * GRID, int(faces.shape[0])
    v0, n0, m0, g0 = vertices.detach(), normals.detach(), looked_up.detach()[..., 5:8], gb.detach()
    tangents, d_v, d_n = torch.empty(V, 4, device=dev), torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
    nbytes = lib.dirt_tangent_scratch_bytes(1, V, F)
    scratch = torch.empty(nbytes // 4, device=dev)
    out, d_g, d_m = torch.empty_like(g0), torch.empty_like(g0), torch.empty(P, P, 3, device=dev)
    head = (v0.data_ptr(), 3, n0.data_ptr(), uvs.data_ptr(), topology.faces.data_ptr(), topology.offsets.data_ptr(), topology.entries.data_ptr())
    tail = (1, P * P, CG, 8, ON, OT, 1., _lib.NORMAL_MAP_ENCODED, stream)
    calls = {
        'tangent_forward': lambda: lib.dirt_tangent_forward(*head, tangents.data_ptr(), 1, V, F, stream),
        'tangent_backward': lambda: lib.dirt_tangent_backward(*head, g_t.data_ptr(), d_v.data_ptr(), d_n.data_ptr(), scratch.data_ptr(), nbytes, 1, V, F, stream),
        'normal_map_forward': lambda: lib.dirt_normal_map_forward(g0.data_ptr(), m0.data_ptr(), out.data_ptr(), *tail),
        'normal_map_backward': lambda: lib.dirt_normal_map_backward(g0.data_ptr(), m0.data_ptr(), g_g.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), *tail),
    }
    for name, call in calls.items():
        assert call() == 0, (name, _lib.last_error())
    c_abi = {name + '_us': timed(call) for name, call in calls.items()}

# what the pixel kernels have to move, per pixel: forward G-buffer in and out and the texel; backward the seven frame channels
# and the texel, grad_out in, d gbuffer and d normal_map out
moved = {'normal_map_forward': 4 * P * P * (2 * CG + 3), 'normal_map_backward': 4 * P * P * (7 + 3 + 2 * CG + 3)}
ratio = lambda a, b: {'forward': results[a][0] / results[b][0], 'backward': results[a][1] / results[b][1]}   # noqa: E731
report = {'workload': 'vertex_tangents: a %d x %d sheet, %d vertices, %d faces; perturb_normals: %d x %d pixels, %d channels (normals at %d, tangents at %d), '
                      'the normal map in place from channels 5:8 of an 8-channel look-up' % (GRID, GRID, GRID * GRID, len(faces_np), P, P, CG, ON, OT),
          'calls_per_figure': 50,
          'public_api_us': {k: {'forward': v[0], 'backward': v[1]} for k, v in results.items()},
          'c_abi_us': c_abi,
          'c_abi_bytes_moved': moved,
          'c_abi_GB_per_s': {k: moved[k] / c_abi[k + '_us'] * 1e-3 for k in moved},
          'ratios': {'torch_over_vertex_tangents': ratio('vertex_tangents_torch', 'vertex_tangents'),
                     'torch_cat_over_perturb_normals': ratio('perturb_normals_torch_cat', 'perturb_normals')}}
print(json.dumps(report))
json.dump(report, open(out_path, 'w'), indent=1)
