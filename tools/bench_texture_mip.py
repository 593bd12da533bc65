"""GPU box: the trilinear texture look-up (dirt_texture_mip.hip) -- HIP-event times of the pyramid build, the forward and the
backward (C ABI calls alone), beside the bilinear forward / backward of tools/bench_texture.py at the same configuration.
The (u, v) field is what a G-buffer holds: smooth, rotated, read in place from channels 1:3 of a 6-channel buffer whose
channel 0 is the mask (all surface here); the level of detail comes from its footprint.  Configurations:
  2048^2 pixels from a 512^2 x 3 texture at scale 4 (~1 texel per pixel) and scale 1 (magnified: lambda = 0);
  512^2 pixels from a 2048^2 x 3 texture at scale 1 (minified: lambda ~ 2).
usage: python tools/bench_texture_mip.py [json path]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import _lib, rasterise_ops as _ops  # noqa: E402

out_path = next((a for a in sys.argv[1:] if a.endswith('.json')), None)
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


results = []
for (H, W, Ht, Wt, Ct, scale) in ((2048, 2048, 512, 512, 3, 4.0), (2048, 2048, 512, 512, 3, 1.0), (512, 512, 2048, 2048, 3, 1.0)):
    rng = np.random.default_rng(0)
    tex = torch.from_numpy(rng.uniform(0, 1, (Ht, Wt, Ct)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((H, W, Ct)).astype(np.float32)).to(dev)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    c, s = np.cos(0.2), np.sin(0.2)
    gbuf = np.zeros((H, W, 6), np.float32)
    gbuf[..., 0] = 1.0
    gbuf[..., 1] = (c * xs / W + s * ys / H) * scale + 0.13
    gbuf[..., 2] = (-s * xs / W + c * ys / H) * scale + 0.41
    gb = torch.from_numpy(gbuf).to(dev)
    uv, mask = gb[..., 1:3], gb[..., 0]
    floats = ctypes.c_longlong(0)
    L = lib.dirt_texture_mip_levels(Ht, Wt, Ct, -1, ctypes.byref(floats))
    pyr = torch.empty(floats.value, device=dev)
    scratch = torch.empty(floats.value, device=dev)
    out = torch.empty((H, W, Ct), device=dev)
    gt = torch.empty_like(tex)
    guv = torch.empty((H, W, 2), device=dev)

    def build():
        assert lib.dirt_texture_mip_build(tex.data_ptr(), pyr.data_ptr(), Ht, Wt, Ct, L, stream) == 0

    def fwd():
        assert lib.dirt_texture_sample_mip_forward(pyr.data_ptr(), uv.data_ptr(), None, mask.data_ptr(), out.data_ptr(), H, W, H, Ht, Wt, Ct, L,
                                                   6, 6, 0.0, 0, stream) == 0

    def bwd():   # clears the scratch pyramid, the tile kernel, the collapse
        assert lib.dirt_texture_sample_mip_backward(pyr.data_ptr(), uv.data_ptr(), None, mask.data_ptr(), g.data_ptr(), scratch.data_ptr(),
                                                    gt.data_ptr(), guv.data_ptr(), None, H, W, H, Ht, Wt, Ct, L, 6, 2, 6, 0.0, 0, stream) == 0

    def bil_fwd():
        assert lib.dirt_texture_sample_forward(tex.data_ptr(), uv.data_ptr(), out.data_ptr(), H * W, Ht, Wt, Ct, 6, 0, stream) == 0

    def bil_bwd():
        assert lib.dirt_texture_sample_backward_image(tex.data_ptr(), uv.data_ptr(), g.data_ptr(), gt.data_ptr(), guv.data_ptr(), H, W, Ht, Wt, Ct,
                                                      6, 2, 0, stream) == 0
    build()
    torch.cuda.synchronize()
    t_build, t_fwd, t_bwd = timed(build), timed(fwd), timed(bwd)
    t_bil_fwd, t_bil_bwd = timed(bil_fwd), timed(bil_bwd)
    r = {'pixels': [H, W], 'texture': [Ht, Wt, Ct], 'scale': scale, 'levels': L, 'texels_per_pixel': Wt * scale / W,
         'build_us': t_build, 'forward_us': t_fwd, 'backward_us': t_bwd,
         'bilinear_forward_us': t_bil_fwd, 'bilinear_backward_us': t_bil_bwd,
         'forward_over_bilinear': t_fwd / t_bil_fwd, 'backward_over_bilinear': t_bwd / t_bil_bwd}
    results.append(r)
    print(json.dumps(r))
if out_path:
    json.dump({'workload': 'trilinear texture look-up, (u, v) and mask in place from a 6-channel G-buffer', 'results': results},
              open(out_path, 'w'), indent=1)
