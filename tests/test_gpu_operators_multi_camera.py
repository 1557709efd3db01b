"""The gsplat-compatible operators with more than one camera: ops.fully_fused_projection, ops.isect_tiles,
ops.isect_offset_encode and ops.rasterize_to_pixels on [C, N, ...] inputs with C = 3.

What only runs with C > 1: cam_id folded into the int64 keys above the tile bits, flatten_ids = cam * N + gaussian,
offset_encode_kernel's fill loops across cameras, camera c rastered through the slice offsets_ext[c * n_tiles:] of one
concatenated offset table over flat [C * N, ...] views, the per-camera background row and its gradient.
Setups (feature_channel_gates.multi_cameras): three ring cameras; the middle camera blind; the last tiles of the last
camera empty.  Lists are compared element for element with the NumPy oracle's; frames go through O.check_frame as in
tests/test_gpu_feature_channels.py, gradients through grad_gate.compare against fp64 autograd over three OT.rasterize
calls, each on its camera's own rows and its own lists (ids without their + c * N, offsets from 0).
"""
import numpy as np
import pytest
import torch

from oracle import gs_oracle_np as O
from feature_channel_gates import (MAX_CH, MULTI, MULTI_CHANNELS, MULTI_SETUPS, BackwardReference, BlendReference,
                                   camera_lists, check_forward, check_lists, cotangents, features, multi_cameras,
                                   multi_camera_lists, scene, tiles_of)
from grad_gate import compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = MULTI["n_cams"]
W, H = MULTI["w"], MULTI["h"]


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def projected(ops):
    """setup -> (g, viewmats, Ks, radii [3,N], means2d, depths, conics): the HIP projection of the three cameras."""
    cache = {}

    def get(setup):
        if setup not in cache:
            g = scene(MULTI)
            cams = multi_cameras(setup)
            vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
            radii, m2d, dep, con, _ = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), vm, Ks, W, H)
            cache[setup] = (g, vm, Ks, radii, m2d, dep, con)
        return cache[setup]
    return get


@pytest.fixture(scope="module")
def blend_refs():
    """fp64 blends by (camera, its projected inputs): the setups share their unchanged cameras."""
    return {}


def _per_axis(radii):
    """Per-axis radii [C,N,2] from [C,N]: the y extent about three quarters of x, both positive or both zero."""
    return np.stack([radii, np.where(radii > 0, (3 * radii + 3) // 4, 0)], axis=-1).astype(np.int32)


@pytest.mark.parametrize("setup", MULTI_SETUPS)
def test_projection_rows_equal_the_single_camera_calls(ops, projected, setup):
    g, vm, Ks, radii, m2d, dep, con = projected(setup)
    assert radii.shape == (C, len(g)) and m2d.shape == (C, len(g), 2) and con.shape == (C, len(g), 3)
    for c in range(C):
        one = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), vm[c:c + 1], Ks[c:c + 1], W, H)
        for name, x, y in zip(("radii", "means2d", "depths", "conics"), (radii, m2d, dep, con), one):
            assert torch.equal(x[c], y[0]), f"camera {c}: {name}"
    vis = (radii > 0).sum(dim=1).tolist()
    assert vis[0] > 0 and vis[2] > 0 and (vis[1] == 0) == (setup == "blind_middle"), vis


@pytest.mark.parametrize("setup", MULTI_SETUPS)
@pytest.mark.parametrize("kind", ["radius", "per_axis"])
def test_isect_tiles_and_offsets_three_cameras(ops, projected, kind, setup):
    g, vm, Ks, radii, m2d, dep, con = projected(setup)
    tw, th = tiles_of(W, H)
    r_np = radii.cpu().numpy() if kind == "radius" else _per_axis(radii.cpu().numpy())
    tpg, keys, ids = ops.isect_tiles(m2d, torch.from_numpy(r_np).to(DEV), dep, 16, tw, th)
    offs = ops.isect_offset_encode(keys, C, tw, th)
    assert tpg.shape == (C, len(g)) and keys.dtype == torch.int64 and ids.dtype == torch.int32
    ref = multi_camera_lists(m2d.cpu().numpy(), r_np, dep.cpu().numpy(), tw, th)
    st = check_lists((tpg.cpu().numpy(), keys.cpu().numpy(), ids.cpu().numpy(), offs.cpu().numpy()), ref, what=f"{setup} {kind}")
    print(f"\n{setup} {kind}: {st}")
    assert st["per_camera"][0] > 0 and st["per_camera"][2] > 0
    if setup == "blind_middle":
        assert st["per_camera"][1] == 0
    if setup == "empty_tail":          # the whole last row of tiles of the last camera is empty
        assert int(offs[2, -1, 0]) == st["n_isect"] and int(offs[2, -1, -1]) == st["n_isect"]


@pytest.mark.parametrize("tw,th", [(1, 1), (2, 1), (1, 3), (2, 2), (7, 1), (4, 2), (3, 3), (9, 7), (16, 4), (13, 5), (31, 33),
                                   (32, 32), (41, 25)])
def test_offset_encode_at_the_edges_of_the_tile_field(ops, tw, th):
    """The key's tile field is floor(log2(n_tiles)) + 1 bits wide; the camera sits above it.  Tile counts of 1, powers of two
    and powers of two +- 1, three cameras of screen-space inputs whose rectangles straddle every image edge: keys, ids and
    offsets equal the oracle's, and an empty key tensor gives all zeros."""
    rng = np.random.default_rng(tw * 100 + th)
    n = 700
    w, h = tw * 16 - int(rng.integers(0, 16)), th * 16 - int(rng.integers(0, 16))
    means2d = np.stack([rng.uniform(-20, w + 20, (C, n)), rng.uniform(-20, h + 20, (C, n))], axis=-1).astype(np.float32)
    radii = rng.choice([0, 0, 1, 3, 8, 17, 40], size=(C, n)).astype(np.int32)
    depths = rng.uniform(0.5, 30.0, (C, n)).astype(np.float32)
    depths[:, rng.integers(0, n, n // 3)] = np.float32(7.25)
    if th > 1:
        radii[2, means2d[2, :, 1] > 0.5 * h] = 0            # the last camera's lower tiles: few or no entries
    tpg, keys, ids = ops.isect_tiles(_t(means2d), torch.from_numpy(radii).to(DEV), _t(depths), 16, tw, th)
    offs = ops.isect_offset_encode(keys, C, tw, th)
    ref = multi_camera_lists(means2d, radii, depths, tw, th)
    st = check_lists((tpg.cpu().numpy(), keys.cpu().numpy(), ids.cpu().numpy(), offs.cpu().numpy()), ref, what=f"{tw}x{th}")
    assert min(st["per_camera"]) > 0
    # the camera field of the last key sits directly above the tile field
    tile_bits = int(np.floor(np.log2(tw * th))) + 1
    assert int(keys[-1]) >> (32 + tile_bits) == C - 1 and (int(keys[-1]) >> 32) & ((1 << tile_bits) - 1) < tw * th
    empty = ops.isect_offset_encode(torch.empty(0, dtype=torch.int64, device=DEV), C, tw, th)
    assert empty.shape == (C, th, tw) and int(empty.abs().max()) == 0
    np.testing.assert_array_equal(empty.cpu().numpy(), O.isect_offsets(np.zeros(0, np.int64), C, tw, th))


@pytest.mark.parametrize("setup", MULTI_SETUPS)
def test_rasterize_to_pixels_three_cameras(ops, projected, blend_refs, setup):
    """Per-camera colours, opacities and backgrounds; each camera's frame against the fp64 blend of its own lists, the
    gradients of L = sum_c <w_c, render_c> + <u_c, alpha_c> against fp64 autograd of the same sum."""
    g, vm, Ks, radii, m2d, dep, con = projected(setup)
    N = len(g)
    tw, th = tiles_of(W, H)
    _, keys, ids = ops.isect_tiles(m2d, radii, dep, 16, tw, th)
    offs = ops.isect_offset_encode(keys, C, tw, th)
    feats_np, _ = features(C * N, seed=13)
    feats_np = feats_np.reshape(C, N, MAX_CH)
    bgs_np = np.stack([features(1, seed=20 + c)[1] for c in range(C)])                  # [C, 32]
    opac_np = np.stack([g.opacities * (1.0 - 0.15 * c) for c in range(C)]).astype(np.float32)
    cots = [cotangents(W, H, seed=30 + c) for c in range(C)]
    m2d_np, con_np = m2d.cpu().numpy(), con.cpu().numpy()
    ids_np, offs_np = ids.cpu().numpy(), offs.cpu().numpy()
    lists = [camera_lists(ids_np, offs_np, c, N) for c in range(C)]
    brefs = [BackwardReference(m2d_np[c], con_np[c], feats_np[c], opac_np[c], lists[c][0], lists[c][1], W, H) for c in range(C)]
    for ch in MULTI_CHANNELS:
        a_m2d, a_con = m2d.detach().clone().requires_grad_(True), con.detach().clone().requires_grad_(True)
        a_col, a_op, a_bg = _t(feats_np[..., :ch], True), _t(opac_np, True), _t(bgs_np[:, :ch], True)
        render, alphas = ops.rasterize_to_pixels(a_m2d, a_con, a_col, a_op, W, H, 16, offs, ids, backgrounds=a_bg, absgrad=True)
        assert render.shape == (C, H, W, ch) and alphas.shape == (C, H, W, 1)
        w_r = torch.stack([_t(cots[c][0][..., :ch]) for c in range(C)])
        w_a = torch.stack([_t(cots[c][1]) for c in range(C)])
        ((render * w_r).sum() + (alphas[..., 0] * w_a).sum()).backward()
        assert a_m2d.absgrad.shape == (C, N, 2) and bool(torch.isfinite(a_m2d.absgrad).all())
        assert bool((a_m2d.absgrad * (1 + 2e-5) + 2e-6 >= a_m2d.grad.abs()).all())
        for c in range(C):
            what = f"{setup} camera {c} ch={ch}"
            if len(lists[c][0]) == 0:            # the blind camera: its frame is its background, its rows get nothing
                assert setup == "blind_middle" and c == 1
                assert torch.equal(render[c].detach(), a_bg[c].detach().expand(H, W, ch)) and float(alphas[c].abs().max()) == 0.0
                for x in (a_m2d.grad[c], a_con.grad[c], a_col.grad[c], a_op.grad[c], a_m2d.absgrad[c]):
                    assert float(x.abs().max()) == 0.0, what
                np.testing.assert_allclose(a_bg.grad[c].cpu().numpy(), cots[c][0][..., :ch].astype(np.float64).sum((0, 1)),
                                           rtol=1e-5, atol=1e-4)
                continue
            key = (c, m2d_np[c].tobytes())
            if key not in blend_refs:
                blend_refs[key] = BlendReference(m2d_np[c], con_np[c], feats_np[c], opac_np[c], lists[c][0], lists[c][1], W, H)
            check_forward(blend_refs[key], ch, render[c].detach().cpu().numpy(), alphas[c, ..., 0].detach().cpu().numpy(),
                          None, bgs_np[c], what=what)
            ref = brefs[c].grads(ch, cots[c][0], cots[c][1], bgs_np[c])
            got = (a_m2d.grad[c], a_con.grad[c], a_col.grad[c], a_op.grad[c].reshape(-1, 1))
            for name, x, r in zip(("v_means2d", "v_conics", "v_colors", "v_opacities"), got, ref):
                st = compare(f"{what} {name}", x, r, bad_frac=5e-3)
                print(f"{what} {name}: {st['rows_over_tol']} of {st['rows']} rows over 2e-3, cosine {st['cosine']:.7f}")
            st = compare(f"{what} v_backgrounds", a_bg.grad[c].reshape(1, -1), ref[4])
            print(f"{what} v_backgrounds: cosine {st['cosine']:.7f}")
        culled = ~(radii > 0)
        assert bool(culled.any()) and float(a_m2d.grad[culled].abs().max()) == 0.0 and float(a_col.grad[culled].abs().max()) == 0.0
