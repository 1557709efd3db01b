"""mgs_deform_apply_sh on the GPU (include/mgs_deform_sh.h, csrc/deform.hip, csrc/sh_rotate.h, robosimgs_amd/deform.py,
FrameRenderer(deform_rotate_sh=)) against the fp64 statement of tests/deform_sh_ref.py.  Every rotated band is held to the
gate counted in that module's docstring (error / bound <= 1; each test prints its worst ratios), everything the header
promises to pass through is compared bit for bit, and the geometry and status are compared bit for bit with
mgs_deform_apply's.  The rotation and its bound are restated on the GPU's own stored binding.

Worst ratios on an MI355X (error / bound): band 1 0.103, band 2 0.040, band 3 0.024, the norm check 0.361; bound_R at most
1.14e-5 (n = 4097 among 12,291 particles); no rotated row without a bound (profiles/deform/README.md).
"""
import math

import numpy as np
import pytest
import torch

import deform_ref as DR
import deform_sh_ref as SR
from test_gpu_deform import DEV, _t, apply_raw, bind_raw, binding_of, cloth_scene, guarded, intact, wave

pytestmark = pytest.mark.gpu
SHAPES = [(1, 4), (2, 9), (3, 16), (1, 16), (0, 16)]             # (degree, stride): both load paths, copied upper coefficients
PATTERN = 0x5A


@pytest.fixture(scope="module")
def D():
    from robosimgs_amd import deform
    return deform


def scene(n, m, seed, kind="cloud"):
    mu, q, s, X = DR.cloud(n, m, seed, kind)
    return mu, q, s, X, dict(means=_t(mu), quats=_t(q), scales=_t(s))


def apply_sh(D, tensors, binding, mode, now, degree, colors, copy_unbound=True, with_status=True, prefill=None):
    """mgs_deform_apply_sh into guarded outputs: (means, quats, scales, status, out_colors) as numpy, guards ok.  prefill: the
    byte out_colors is filled with before the call."""
    n = binding.n
    om, gm = guarded((n, 3), torch.float32)
    oq, gq = guarded((n, 4), torch.float32)
    osc, gs = guarded((n, 3), torch.float32)
    oc, gc = guarded(tuple(colors.shape), torch.float32)
    if prefill is not None:
        oc.view(torch.uint8).fill_(prefill)
    st, gst = guarded((n,), torch.uint8) if with_status else (None, None)
    D.deform_apply_sh_raw(tensors["means"], tensors["quats"], tensors["scales"], binding, mode, now, om, oq, osc, degree, colors,
                          oc, copy_unbound, status=st)
    torch.cuda.synchronize()
    ok = intact(gm, gq, gs, gc) and (gst is None or intact(gst))
    return om.cpu().numpy(), oq.cpu().numpy(), osc.cpu().numpy(), (st.cpu().numpy() if with_status else None), oc.cpu().numpy(), ok


def worse(worst, res):
    for k, v in res.items():
        if k != "rotated":
            worst[k] = max(worst.get(k, 0.0), v)


def passes(res):
    return all(v <= 1.0 for k, v in res.items() if k.startswith("band") or k == "norm")


# ---- 1. against fp64, at the wave and workgroup edges ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_apply_sh_against_fp64(D, n, mode):
    m = max(64, 3 * n)
    mu, q, s, X, tensors = scene(n, m, 10 * n + mode)
    select = np.ones(n, np.uint8)
    select[3::7] = 0                                                     # unbound rows (none when n = 1)
    arrays, ok = bind_raw(D, mu, X, select)
    assert ok
    binding = binding_of(D, arrays, m)
    idx, flags = arrays[0], arrays[4]
    unbound = (flags & 1) != 0
    cols = {stride: SR.random_colors(n, stride, n + stride) for stride in (4, 9, 16)}
    worst, rotated = {}, 0
    for motion in ("rigid", "bend", "stretch"):
        Y = DR.move(X, motion, seed=n)
        victim = int(idx[2, 0])                                          # a neighbour of Gaussian 0 blows up at frame time
        Y[victim] = (np.nan, np.inf)[mode], 0.0, 0.0
        now = _t(Y)
        gm, gq, gs, gst, ok = apply_raw(D, tensors, binding, mode, now)  # mgs_deform_apply: the geometry to equal
        assert ok
        ref = DR.apply_ref(mu, q, s, *arrays, mode, Y, status_seen=gst)
        assert (gst[unbound] == DR.ST_UNBOUND).all() and gst[0] == (DR.ST_NONFINITE if not unbound[0] else DR.ST_UNBOUND)
        for degree, stride in SHAPES:
            c = cols[stride]
            ct = _t(c)
            om, oq, osc, st, oc, ok = apply_sh(D, tensors, binding, mode, now, degree, ct, prefill=PATTERN)
            assert ok, "a guard band was written"
            assert om.tobytes() == gm.tobytes() and oq.tobytes() == gq.tobytes() and osc.tobytes() == gs.tobytes()
            assert st.tobytes() == gst.tobytes()
            res = SR.check_sh(ref, q, c, oc, degree)
            worse(worst, res)
            assert passes(res), (motion, degree, stride, res)
            if degree >= 1:
                rotated = max(rotated, res["rotated"])
                assert res["rotated"] == int(((gst & (DR.ST_UNBOUND | DR.ST_THIN | DR.ST_NONFINITE)) == 0).sum())
            else:
                assert oc.tobytes() == c.tobytes()                       # degree 0 rotates nothing
            # the same bytes again, with and without status
            om2, oq2, osc2, st2, oc2, ok2 = apply_sh(D, tensors, binding, mode, now, degree, ct, with_status=False, prefill=0)
            assert ok2 and st2 is None and oc2.tobytes() == oc.tobytes()
            assert om2.tobytes() == gm.tobytes() and oq2.tobytes() == gq.tobytes() and osc2.tobytes() == gs.tobytes()
            # copy_unbound = 0: unbound rows keep what the buffer held, every bound row is written as before
            om3, oq3, osc3, st3, oc3, ok3 = apply_sh(D, tensors, binding, mode, now, degree, ct, copy_unbound=False, prefill=PATTERN)
            assert ok3 and st3.tobytes() == gst.tobytes() and om3.tobytes() == gm.tobytes()
            assert (oc3[unbound].view(np.uint8) == PATTERN).all() and oc3[~unbound].tobytes() == oc[~unbound].tobytes()
    if n >= 63:
        assert rotated > n // 2
    print(f"\napply_sh n {n} mode {mode}: {rotated} rows rotate, worst ratios {worst}")


# ---- 2. degenerate neighbourhoods ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["strand", "sheet"])
def test_apply_sh_on_degenerate_neighbourhoods(D, kind):
    n, m = 300, 500
    mu, q, s, X, tensors = scene(n, m, 77, kind)
    arrays, ok = bind_raw(D, mu, X)
    binding = binding_of(D, arrays, m)
    c = SR.random_colors(n, 16, 5)
    Y = DR.move(X, "bend")
    rows = {}
    for mode in (0, 1):
        gm, gq, gs, gst, ok0 = apply_raw(D, tensors, binding, mode, _t(Y))
        om, oq, osc, st, oc, ok = apply_sh(D, tensors, binding, mode, _t(Y), 3, _t(c), prefill=PATTERN)
        assert ok and ok0 and om.tobytes() == gm.tobytes() and oq.tobytes() == gq.tobytes() and osc.tobytes() == gs.tobytes()
        assert st.tobytes() == gst.tobytes()
        ref = DR.apply_ref(mu, q, s, *arrays, mode, Y, status_seen=st)
        res = SR.check_sh(ref, q, c, oc, 3)
        print(f"\n{kind} mode {mode}: {res}, status {np.bincount(st, minlength=9).tolist()}")
        assert passes(res), res
        rows[mode] = oc
        if kind == "strand":                                             # all thin: every row is the input's bits
            assert (st == DR.ST_THIN).all() and res["rotated"] == 0 and oc.tobytes() == c.tobytes()
        else:                                                            # cloth: all rotate; in mode 1 all fall back, and rotate
            assert (st == (0 if mode == 0 else DR.ST_FALLBACK)).all() and res["rotated"] == n
    assert rows[0].tobytes() == rows[1].tobytes()                        # colours are the same in mode 0 and mode 1


def test_colours_are_the_same_in_both_modes_and_bound_rows_are_rewritten(D):
    n, m = 257, 800
    mu, q, s, X, tensors = scene(n, m, 31)
    select = np.ones(n, np.uint8)
    select[::5] = 0
    arrays, _ = bind_raw(D, mu, X, select)
    binding = binding_of(D, arrays, m)
    unbound = (arrays[4] & 1) != 0
    c = SR.random_colors(n, 16, 9)
    moved = DR.move(X, "bend")
    a0 = apply_sh(D, tensors, binding, 0, _t(moved), 3, _t(c))
    a1 = apply_sh(D, tensors, binding, 1, _t(moved), 3, _t(c))
    assert a0[5] and a1[5] and (a1[3][~unbound] == 0).mean() > 0.9        # mode 1: affine rows that did not fall back
    assert a0[4].tobytes() == a1[4].tobytes() and a0[2].tobytes() != a1[2].tobytes()
    # frame A (moved), then frame B (the rest positions) into the SAME buffer with copy_unbound = 0: every bound row is
    # rewritten, so it returns to its rest row within the bound of R ~ I, and the unbound rows keep the buffer's bytes
    om = torch.empty(n, 3, device=DEV)
    oq, osc, oc = torch.empty(n, 4, device=DEV), torch.empty(n, 3, device=DEV), torch.empty(n, 16, 3, device=DEV)
    oc.view(torch.uint8).fill_(PATTERN)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    args = (tensors["means"], tensors["quats"], tensors["scales"], binding, 0)
    D.deform_apply_sh_raw(*args, _t(moved), om, oq, osc, 3, _t(c), oc, False, status=st)
    frame_a = oc.cpu().numpy()
    assert frame_a[~unbound].tobytes() == a0[4][~unbound].tobytes()
    D.deform_apply_sh_raw(*args, _t(X), om, oq, osc, 3, _t(c), oc, False, status=st)
    frame_b, st_b = oc.cpu().numpy(), st.cpu().numpy()
    assert (frame_b[unbound].view(np.uint8) == PATTERN).all()
    ref = DR.apply_ref(mu, q, s, *arrays, 0, X, status_seen=st_b)
    R, bR = SR.rotation_of(ref, q)
    rows = SR.rotated_rows(ref)
    assert rows[~unbound].all()
    off_I = np.linalg.norm(R[rows] - np.eye(3), axis=(1, 2))               # R_ref of the rest positions: I to the rounding of w and p
    assert off_I.max() <= 1e-4
    res = SR.check_sh(ref, q, c, frame_b, 3, written=~unbound)
    print(f"\nframe B at the rest positions: {res}")
    assert passes(res) and res["rotated"] == int((~unbound).sum())
    for l in (1, 2, 3):                                                  # back at the rest row, and away from frame A's
        sl = slice(l * l, (l + 1) * (l + 1))
        cn = np.linalg.norm(c[rows, sl].astype(np.float64), axis=1)
        back = np.linalg.norm(frame_b[rows, sl].astype(np.float64) - c[rows, sl], axis=1)
        assert (back <= (1.01 * l * (bR[rows] + off_I)[:, None] / np.sqrt(2) + SR.A[l]) * cn).all()      # the gate, and M_l(R_ref) ~ I
        away = np.linalg.norm(frame_a[rows, sl].astype(np.float64) - c[rows, sl], axis=1)
        assert np.median(away / np.maximum(cn, 1e-30)) > 1e-2


# ---- 3. deform_gaussians ---------------------------------------------------------------------------------------------------
def test_deform_gaussians_rotate_sh_contract(D):
    n, m = 500, 600
    mu, q, s, X, tensors = scene(n, m, 3)
    c = SR.random_colors(n, 16, 2)
    tensors.update(opacities=torch.full((n,), 0.5, device=DEV), colors=_t(c), sh_degree=3)
    binding = D.bind_particles(tensors["means"], _t(X), select=_t(np.arange(n) % 4 != 0, np.uint8))
    now = _t(DR.move(X, "bend"))
    plain = D.deform_gaussians(tensors, binding, now)                     # today's dict: shared colours
    off = D.deform_gaussians(tensors, binding, now, rotate_sh=False)
    assert plain["colors"] is tensors["colors"] and off["colors"] is tensors["colors"] and off["opacities"] is tensors["opacities"]
    raw = apply_raw(D, tensors, binding, 0, now)
    assert off["means"].cpu().numpy().tobytes() == raw[0].tobytes() and off["quats"].cpu().numpy().tobytes() == raw[1].tobytes()
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    on = D.deform_gaussians(tensors, binding, now, rotate_sh=True, status=st)
    want = apply_sh(D, tensors, binding, 0, now, 3, tensors["colors"])
    assert on["colors"].data_ptr() != tensors["colors"].data_ptr() and on["colors"].cpu().numpy().tobytes() == want[4].tobytes()
    assert on["means"].cpu().numpy().tobytes() == raw[0].tobytes() and st.cpu().numpy().tobytes() == raw[3].tobytes()
    assert on["sh_degree"] == 3 and torch.equal(tensors["colors"], _t(c))  # the rest rows survive
    # out= reuse: the previous result's buffers, colours included
    again = D.deform_gaussians(tensors, binding, now, rotate_sh=True, out=on)
    assert all(again[k].data_ptr() == on[k].data_ptr() for k in ("means", "quats", "scales", "colors"))
    # copy_unbound=False on a reused buffer leaves the unbound rows alone
    unbound = (binding.flags & 1) != 0
    on["colors"][unbound] = 7.0
    kept = D.deform_gaussians(tensors, binding, now, rotate_sh=True, out=on, copy_unbound=False)
    assert kept["colors"].data_ptr() == on["colors"].data_ptr() and bool((kept["colors"][unbound] == 7.0).all())
    assert kept["colors"][~unbound].cpu().numpy().tobytes() == want[4][~unbound.cpu().numpy()].tobytes()
    # out carrying the rest's colours (a rotate_sh=False result): a new tensor, fully written even with copy_unbound=False
    fresh = D.deform_gaussians(tensors, binding, now, rotate_sh=True, out=off, copy_unbound=False)
    assert fresh["colors"].data_ptr() != tensors["colors"].data_ptr() and fresh["means"].data_ptr() == off["means"].data_ptr()
    assert fresh["colors"].cpu().numpy().tobytes() == want[4].tobytes()
    # degree 0, or rows too short for the degree: the call without SH, colours shared
    flat = D.deform_gaussians(dict(tensors, sh_degree=0), binding, now, rotate_sh=True)
    assert flat["colors"] is tensors["colors"]
    short = dict(tensors, colors=tensors["colors"][:, :9].contiguous())
    assert D.deform_gaussians(short, binding, now, rotate_sh=True)["colors"] is short["colors"]


# ---- 4. graph capture ------------------------------------------------------------------------------------------------------
def test_apply_sh_replays_in_a_graph(D):
    n, m = 1000, 800
    mu, q, s, X, tensors = scene(n, m, 21)
    tensors.update(opacities=torch.full((n,), 0.5, device=DEV), colors=_t(SR.random_colors(n, 16, 1)), sh_degree=3)
    binding = D.bind_particles(tensors["means"], _t(X))
    frames = [_t(DR.move(X, motion, seed=k)) for k, motion in enumerate(("rigid", "bend", "stretch"))]
    keys = ("means", "quats", "scales", "colors")
    eager = []
    for f in frames:
        o = D.deform_gaussians(tensors, binding, f, mode="affine", rotate_sh=True)
        eager.append([o[k].clone() for k in keys])
    assert not torch.equal(eager[0][3], eager[1][3])
    now = frames[0].clone()
    out = {k: torch.empty_like(tensors[k]) for k in keys}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        D.deform_gaussians(tensors, binding, now, mode="affine", rotate_sh=True, out=out)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = D.deform_gaussians(tensors, binding, now, mode="affine", rotate_sh=True, out=out)
        assert all(res[k].data_ptr() == out[k].data_ptr() for k in keys)
        for k in (1, 2, 0):
            now.copy_(frames[k])
            for v in out.values():
                v.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for key, want in zip(keys, eager[k]):
                assert out[key].cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (k, key)
    torch.cuda.synchronize()


# ---- 5. FrameRenderer(deform_rotate_sh=) -------------------------------------------------------------------------------------
def sh_cloth_scene():
    tensors, parts, soft, vm, K = cloth_scene()                            # 18 x 18 Gaussians per side, 12 x 12 particles
    n = tensors["means"].shape[0]
    c = SR.random_colors(n, 16, 12)
    c[:, 0] += 0.8
    return dict(tensors, colors=_t(c), sh_degree=3), parts, soft, vm, K


def test_frame_renderer_rotates_sh_per_frame(D):
    from robosimgs_amd import FrameRenderer, rasterization, transform_gaussians
    tensors, parts, soft, vm, K = sh_cloth_scene()
    binding = D.bind_particles(tensors["means"], _t(parts), select=_t(soft, np.uint8))
    kw = dict(render_mode="RGB+ED", frames_in_flight=2, isect_capacity=200_000, deform=binding, deform_mode="rigid")
    r = FrameRenderer(tensors, 64, 64, deform_rotate_sh=True, **kw)
    assert r.deform_rotate_sh

    def raster(posed):
        return rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"], _t(vm)[None],
                             _t(K)[None], 64, 64, sh_degree=3, render_mode="RGB+ED")

    def by_hand(x, renderer, rotate_sh, group_pose=None):
        posed = D.deform_gaussians(renderer.t, renderer.deform, _t(x), mode=renderer.deform_mode, rotate_sh=rotate_sh)
        if group_pose is not None:
            posed = transform_gaussians(posed, *group_pose, group_ids=renderer.group_ids, rotate_sh=True)
        return raster(posed)

    def frame(renderer, **submit):
        tk = renderer.submit(vm, K, **submit)
        f = renderer.fetch(tk)
        got = f["colors"].clone(), f["alphas"].clone()
        renderer.release(tk)
        return got

    frames = [wave(parts, 0.7 * k) for k in range(1, 5)]
    turned = 0
    for x in frames:                                                       # two slots, four frames: every slot is reused
        c, a = frame(r, particles=x)
        wc, wa, _ = by_hand(x, r, True)
        assert torch.equal(c, wc[0]) and torch.equal(a, wa[0])
        turned += int(not torch.equal(c, by_hand(x, r, False)[0][0]))
    assert turned == 4                                                     # the rotation shows in the pixels

    # deform_rotate_sh=False is the renderer built without the keyword, bit for bit
    off, plain = FrameRenderer(tensors, 64, 64, deform_rotate_sh=False, **kw), FrameRenderer(tensors, 64, 64, **kw)
    assert not off.deform_rotate_sh and not plain.deform_rotate_sh
    for x in frames:
        (c0, a0), (c1, a1) = frame(off, particles=x), frame(plain, particles=x)
        wc, wa, _ = by_hand(x, plain, False)
        assert torch.equal(c0, c1) and torch.equal(a0, a1) and torch.equal(c1, wc[0])

    # with group_ids as well, both rotations on: the group transform turns its rows in place on the slot's copy, which
    # would hold last frame's rotated rows unless the deformation rewrote them from the rest rows (copy_unbound)
    gid = torch.where(_t(soft, np.uint8) != 0, -1, 0).to(torch.int32)
    both = FrameRenderer(tensors, 64, 64, render_mode="RGB+ED", frames_in_flight=1, isect_capacity=200_000, deform=binding,
                         deform_mode="affine", deform_rotate_sh=True, group_ids=gid, n_groups=1, rotate_sh=True)
    for k, x in enumerate(frames):
        ang = 0.5 + 0.4 * k
        Rz = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1.0]])
        Rx = np.array([[1.0, 0, 0], [0, math.cos(ang), -math.sin(ang)], [0, math.sin(ang), math.cos(ang)]])
        pose = ([Rz @ Rx], [[0.2 - 0.05 * k, -0.1, 0.0]])
        c, a = frame(both, rotations=pose[0], translations=pose[1], particles=x)
        wc, wa, _ = by_hand(x, both, True, pose)
        assert torch.equal(c, wc[0]) and torch.equal(a, wa[0]), k
        assert not torch.equal(c, by_hand(x, both, True)[0][0])            # the block moved
