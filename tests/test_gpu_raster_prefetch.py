"""The candidate loop of raster_kernel_v2 (dirt_amd/csrc/dirt_forward.hip) where a rewritten loop can go wrong: waves with
0, 1, 2 and 3 candidates, a tile whose candidates fill one 64-candidate group or a whole round exactly and with one to spare,
a candidate that touches only the second block of a wave's region, samples in the undecided strip (the f64 test is called in
the middle of a visit), equal depths, a frame that is no multiple of the tile, non-finite vertices; 1, 3 and 4 channels and
the visibility pass; the four- and the eight-wave shape, pinned.  Pixels -- and for the visibility pass the face ids --
bit for bit against the CPU oracle."""
import functools

import numpy as np
import pytest
import torch

from dirt_amd import _lib, rasterise_ops as ops
from tests import scenes

pytestmark = pytest.mark.gpu

# 32 x 32-pixel tiles pinned (small frames would take 16 x 16 tiles and another kernel): four waves per tile, or eight
SHAPES = [pytest.param(_lib.FLAG_TILES_LARGE, id='four-waves'), pytest.param(_lib.FLAG_TILES_LARGE | _lib.FLAG_TILES_SMALL, id='eight-waves')]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(H, W, C, tris, seed, extra_vertices=()):
    """tris: [((x, y) * 3, z)] in image coordinates -- x to the right, y DOWN from the top edge, pixel centres at .5 -- drawn
    flat at clip-space depth z (w = 1).  extra_vertices: three more rows [x, y, z, w] per extra face, taken as they are."""
    rng = np.random.default_rng(seed)
    v = []
    for pts, z in tris:
        for x, y in pts:
            v.append((2.0 * x / W - 1.0, 2.0 * (H - y) / H - 1.0, z, 1.0))
    v.extend(extra_vertices)
    vertices = np.asarray(v, np.float32).reshape(-1, 4)
    V = vertices.shape[0]
    return dict(background=rng.uniform(0, 1, (H, W, C)).astype(np.float32), vertices=vertices,
                vertex_colors=rng.uniform(0, 1, (V, C)).astype(np.float32), faces=np.arange(V, dtype=np.int32).reshape(-1, 3),
                height=H, width=W, channels=C)


def _corner(x, y, size, z):
    """A right triangle with its legs along the pixel grid, strictly inside [x, x + size] x [y, y + size]."""
    return (((x + 0.25, y + 0.25), (x + size - 0.25, y + 0.25), (x + 0.25, y + size - 0.25)), z)


def _counts_tris():
    """One 32 x 32 tile.  Candidates per 16 x 8 region of the eight-wave shape (wx, wy): (1, 0): one -- in the region's SECOND
    8 x 8 block only --, (0, 2): two, (1, 3): three, none anywhere else; per 16 x 16 region of the four-wave shape therefore
    (0, 0): none, (1, 0): one (its block (1, 0) only), (0, 1): two, (1, 1): three.  Every triangle keeps a pixel's distance
    from its region's border, so its pixel box cannot reach a neighbour."""
    tris = [_corner(16 + 9, 1, 5, 0.1)]
    tris += [_corner(1 + 4 * j, 16 + 1, 6, 0.2 - 0.1 * j) for j in range(2)]
    tris += [_corner(16 + 1 + 3 * j, 24 + 1, 6, 0.3 * (j - 1)) for j in range(3)]
    return tris


def _cluster_tris(n, seed, size=32):
    """n small triangles, every one of them inside the first 32 x 32 tile and wide enough to hold a pixel centre: the tile has
    exactly n candidates."""
    rng = np.random.default_rng(seed)
    tris = []
    for _ in range(n):
        x, y = rng.uniform(1.0, 24.0, 2)
        tris.append((((x, y), (x + rng.uniform(3.0, 6.0), y + rng.uniform(0.0, 1.0)), (x + rng.uniform(0.0, 1.0), y + rng.uniform(3.0, 6.0))),
                     float(rng.uniform(-0.8, 0.8))))
    return tris


@functools.lru_cache(maxsize=None)
def _case(name, C):
    """(scene, the oracle's pixels, the oracle's face ids), built once per (case, channel count) and shared by the shapes."""
    import oracle
    oracle.build()
    if name == 'counts':
        s = _scene(32, 32, C, _counts_tris(), 1)
    elif name.startswith('cluster'):       # 64 / 65: the loop's second 64-candidate group; 96 / 97: a round's capacity, the slots reused
        n = int(name[7:])
        frame = 32 if n <= 65 else 64
        far = [_corner(40, 40, 9, 0.5), _corner(3, 45, 12, -0.2)] if frame == 64 else []   # (the other tiles are not empty)
        s = _scene(frame, frame, C, _cluster_tris(n, n) + far, n)
    elif name == 'undecided':              # the reference's flat quad, its sides and its diagonal THROUGH pixel centres
        q = [(8.5, 8.5), (8.5, 24.5), (24.5, 24.5), (24.5, 8.5)]
        s = _scene(32, 32, C, [((q[0], q[1], q[2]), 0.0), ((q[0], q[2], q[3]), 0.0)], 2)
    elif name == 'ties':                   # equal depth: the lower face index wins, drawn first (large under small) or second
        big, small = lambda x, y: _corner(x, y, 13, 0.25), lambda x, y: _corner(x + 1, y + 1, 7, 0.25)
        s = _scene(32, 32, C, [big(1, 1), small(1, 1), small(17, 17), big(17, 17)], 3)
    elif name == 'odd-frame':
        s = scenes.rand_scene(80, 17, 33, C, 4, 0.05, 0.4)
    elif name == 'non-finite':             # a NaN, an inf and an enormous face among the hand-placed ones
        extra = [(np.nan, 0.0, 0.0, 1.0), (0.3, 0.3, 0.0, 1.0), (0.1, 0.5, 0.0, 1.0),
                 (np.inf, 0.0, 0.0, 1.0), (0.3, -0.3, 0.0, 1.0), (0.1, -0.5, 0.0, 1.0),
                 (0.2, -np.inf, 0.0, 1.0), (-0.3, -0.3, np.nan, 1.0), (0.1, 0.5, 0.0, np.inf),
                 (-1e6, -1e6, 0.7, 1.0), (1e6, -1e6, 0.7, 1.0), (0.0, 1e6, 0.7, 1.0)]
        s = _scene(32, 32, C, _counts_tris(), 5, extra)
    else:
        raise KeyError(name)
    want = oracle.forward(s['background'][None], s['vertices'][None], s['vertex_colors'][None], s['faces'][None])
    want.setflags(write=False)
    fid = oracle.visibility(s['vertices'], s['faces'], s['height'], s['width'])[0]
    fid.setflags(write=False)
    return s, want, fid


def _visibility(s, dev, flags):
    """ops._op_visibility with the tile shape pinned (the op itself takes no flags)."""
    lib = _lib.load()
    v, f = ops._dense16(_t(s['vertices'][None], dev)), ops._dense16(_t(s['faces'][None], dev))
    H, W = s['height'], s['width']
    face_id = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    with ops._on_device(dev):
        ws = ops._workspace(dev, lib.dirt_workspace_bytes(1, v.shape[1], f.shape[1], H, W, 1))
        _lib.check(lib.dirt_rasterise_visibility(v.data_ptr(), f.data_ptr(), face_id.data_ptr(), 1, v.shape[1], f.shape[1], H, W,
                                                 ws.data_ptr(), ws.numel(), flags, ops._stream_handle(dev)))
    return face_id[0].cpu().numpy()


CASES = [('counts', 1), ('counts', 3), ('counts', 4), ('cluster64', 4), ('cluster65', 4), ('cluster65', 3), ('cluster96', 4), ('cluster97', 4),
         ('cluster97', 1), ('undecided', 1), ('undecided', 4), ('ties', 3), ('ties', 4), ('odd-frame', 1), ('odd-frame', 3), ('odd-frame', 4),
         ('non-finite', 4)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('name,C', CASES)
def test_pixels_bit_exact(gpu, name, C, shape):
    s, want, _ = _case(name, C)
    got = ops._op_rasterise(_t(s['background'][None], gpu), _t(s['vertices'][None], gpu), _t(s['vertex_colors'][None], gpu),
                            _t(s['faces'][None], gpu), s['height'], s['width'], C, flags=shape).cpu().numpy()
    assert got.shape == want.shape
    nbad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    assert nbad == 0, '%s, %d channels: %d of %d pixel values differ from the oracle' % (name, C, nbad, got.size)


@pytest.mark.parametrize('name', ['counts', 'cluster64', 'cluster65', 'cluster96', 'cluster97', 'undecided', 'ties', 'odd-frame', 'non-finite'])
def test_visibility_face_ids(gpu, name):
    """The visibility pass (four waves per tile, no colours) over the same scenes."""
    s, _, fid = _case(name, 1)
    got = _visibility(s, gpu, _lib.FLAG_TILES_LARGE)
    nbad = int(np.sum(got != fid))
    assert nbad == 0, '%s: %d of %d face ids differ from the oracle' % (name, nbad, got.size)


def test_the_scenes_are_what_they_claim():
    """(no GPU needed -- but marked with the file) every hand-placed face is the front-most one somewhere: none was dropped as
    degenerate or culled, so the candidate counts above are the counts the kernel sees."""
    for name in ('counts', 'cluster64', 'cluster65', 'cluster96', 'cluster97', 'ties'):
        s, _, fid = _case(name, 1)
        n = s['faces'].shape[0]
        if name.startswith('cluster'):   # a small triangle may lie wholly behind others: its pixel box must hold a pixel centre
            v = s['vertices'].reshape(n, 3, 4)
            W, H = s['width'], s['height']
            x = (v[:, :, 0] + 1.0) * 0.5 * W
            y = (v[:, :, 1] + 1.0) * 0.5 * H
            assert np.all(np.floor(x.max(1) - 0.5) >= np.ceil(x.min(1) - 0.5)) and np.all(np.floor(y.max(1) - 0.5) >= np.ceil(y.min(1) - 0.5))
            n_tile = int(np.sum((x.max(1) < 32.0) & (H - y.min(1) < 32.0)))
            assert n_tile == int(name[7:]), (name, n_tile)
        else:
            seen = set(np.unique(fid).tolist())
            assert set(range(n)) <= seen | ({1} if name == 'ties' else set()), (name, sorted(seen))
