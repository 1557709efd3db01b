"""Particle-driven deformation on the GPU (include/mgs_deform.h, csrc/deform.hip, robosimgs_amd/deform.py) against the fp64
statement of tests/deform_ref.py.  Every value is held to the bound counted in that module's docstring (the gate is error /
bound <= 1 everywhere; each test prints its worst ratios), indices on an integer lattice and everything the header
promises to pass through are compared bit for bit.  Each stage is held on its own: the bind at the neighbour indices the
GPU chose, the apply on the GPU's own stored binding.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import deform_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "deform.hip")).read()
_const = lambda name: int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, SRC).group(1))
G, T = _const("kDeformGroup"), _const("kDeformTile")
GUARD = 256


@pytest.fixture(scope="module")
def D():
    from robosimgs_amd import deform
    return deform


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def guarded(shape, dtype):
    """A tensor of `shape` followed by GUARD bytes of 0xA5: (tensor, guard)."""
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf[:nbytes].view(dtype).view(shape), buf[nbytes:]


def intact(*guards):
    return all(bool((g == 0xA5).all().item()) for g in guards)


def bind_raw(D, means, parts, select=None, max_distance=math.inf, fill=0xA5):
    """mgs_deform_bind into guarded outputs with a workspace filled with `fill`: (numpy idx, w, p, rest, flags), guards ok."""
    n, m = means.shape[0], parts.shape[0]
    outs = [guarded((DR.K, n), torch.int32), guarded((DR.K, n), torch.float32), guarded((DR.K, 3, n), torch.float32),
            guarded((DR.REST_ROWS, n), torch.float32), guarded((n,), torch.uint8)]
    ws_bytes = D.bind_workspace_bytes(n, m)
    ws = torch.full((ws_bytes + 256 + GUARD,), fill, dtype=torch.uint8, device=DEV)
    pad = -ws.data_ptr() % 256
    tail = ws[pad + ws_bytes:].clone()
    sel = None if select is None else _t(select, np.uint8)
    D.deform_bind_raw(_t(means), _t(parts), sel, max_distance, *[o[0] for o in outs], workspace=ws[:pad + ws_bytes])
    torch.cuda.synchronize()
    ok = intact(*[o[1] for o in outs]) and torch.equal(ws[pad + ws_bytes:], tail)
    return [o[0].cpu().numpy() for o in outs], ok


def binding_of(D, arrays, m, parts=None):
    idx, w, p, rest, flags = arrays
    return D.ParticleBinding(_t(idx, np.int32), _t(w), _t(p), _t(rest), _t(flags, np.uint8), idx.shape[1], m,
                             None if parts is None else _t(parts))


# ---- 1. the neighbour search on an integer lattice: exact distances, ties everywhere -----------------------------------------
def lattice(n, m, seed):
    rng = np.random.default_rng(seed)
    side = max(2, int(math.ceil(m ** (1.0 / 3.0))))
    pts = np.array([[i, j, k] for i in range(side) for j in range(side) for k in range(side)], np.float32)
    parts = pts[rng.permutation(len(pts))[:m]]                             # the index order is not the lattice order
    means = (rng.integers(0, 2 * side - 1, (n, 3)) * 0.5).astype(np.float32)      # lattice and half-lattice points
    return means, parts


@pytest.mark.parametrize("m", [8, 9, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_bind_on_an_integer_lattice_gives_the_reference_indices_bit_for_bit(D, n, m):
    means, parts = lattice(n, m, 1000 * n + m)
    Dx = DR.d2_exact(means, parts)
    assert np.array_equal(Dx, DR.d2_fp32(means, parts))                  # every d2 is exact in fp32
    want, d = DR.knn_ref(Dx)
    ties = int((np.sort(Dx, axis=1)[:, DR.K - 1] == np.sort(Dx, axis=1)[:, min(DR.K, m - 1)]).sum()) if m > DR.K else 0
    (idx, w, p, rest, flags), ok = bind_raw(D, means, parts)
    assert ok, "a guard band was written"
    assert np.array_equal(idx, want), np.flatnonzero((idx != want).any(0))[:8]
    assert np.array_equal(rest[9], d[DR.K - 1].astype(np.float32))       # h^2 = d2_7, exact here
    ref = DR.bind_ref(means, parts, idx)
    ratios = DR.check_bind(ref, w, p, rest, flags)
    print(f"\nlattice n {n} m {m}: {ties} Gaussians with a tie across the 8th place, ratios {ratios}, "
          f"free flags {int((ref['flags_free'] != 0).sum())}")
    assert m == 8 or n < 63 or ties > 0
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ---- 2. random clouds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,kind", [(1000, 3 * T + 5, "cloud"), (G + 1, T + 1, "cloud"), (700, 900, "sheet"), (300, 500, "strand")])
def test_bind_on_random_clouds(D, n, m, kind):
    means, _, _, parts = DR.cloud(n, m, n + m, kind)
    (idx, w, p, rest, flags), ok = bind_raw(D, means, parts)
    assert ok and (idx >= 0).all() and (idx < m).all()
    worst = DR.check_neighbours(means, parts, idx)
    ref = DR.bind_ref(means, parts, idx)
    ratios = DR.check_bind(ref, w, p, rest, flags)
    print(f"\n{kind} n {n} m {m}: neighbour choice {worst:.3f}, ratios {ratios}, flags {np.bincount(flags, minlength=8).tolist()}, "
          f"free flags {int((ref['flags_free'] != 0).sum())}")
    assert worst <= 1.0 and all(v <= 1.0 for v in ratios.values()), (worst, ratios)
    if kind == "cloud":
        assert (flags & DR.FLAG_THIN == 0).all() and (flags & DR.FLAG_FLAT != 0).mean() < 0.01
    elif kind == "sheet":
        assert (flags == DR.FLAG_FLAT).all() and not rest[3:9].any()
    else:
        assert (flags & DR.FLAG_THIN != 0).all()


# ---- 3. eligibility and determinism ------------------------------------------------------------------------------------------
def test_bind_eligibility_and_determinism(D):
    n, m = 2 * G + 3, T + 9
    means, _, _, parts = DR.cloud(n, m, 5)
    rng = np.random.default_rng(0)
    select = (rng.random(n) < 0.7).astype(np.uint8)
    select[:G] = 0                                                       # a whole workgroup without an eligible Gaussian
    means[[G + 1, n - 1]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    parts[[0, T - 1, T, m - 1]] = [[np.nan, 0, 0], [0, -np.inf, 0], [0, 0, np.inf], [np.nan, np.nan, np.nan]]
    nearest = np.sqrt(np.sort(DR.d2_exact(means, parts), axis=1)[:, 0])
    v = np.sort(nearest[np.isfinite(nearest)])
    md = float(0.5 * (v[len(v) // 2] + v[len(v) // 2 + 1]))              # between two Gaussians' nearest distances
    assert np.abs(nearest - md).min() > 1e-6                              # nobody sits on the limit
    (a, ok_a) = bind_raw(D, means, parts, select, md, fill=0xA5)
    (b, ok_b) = bind_raw(D, means, parts, select, md, fill=0x00)
    assert ok_a and ok_b
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()                                 # nothing in the workspace reaches the outputs
    idx, w, p, rest, flags = a
    want, _ = DR.knn_ref(DR.d2_exact(means, parts), select, md)
    unbound = want[0] < 0
    assert unbound[:G].all() and unbound[G + 1] and unbound[n - 1] and 0 < unbound.sum() < n
    assert np.array_equal(flags & 1, unbound.astype(np.uint8))
    assert (idx[:, unbound] == -1).all() and not w[:, unbound].any() and not p[:, :, unbound].any() and not rest[:, unbound].any()
    assert (flags[unbound] == DR.FLAG_UNBOUND).all()
    bad = {0, T - 1, T, m - 1}
    assert not bad & set(idx[:, ~unbound].reshape(-1).tolist())
    assert DR.check_neighbours(means, parts, idx) <= 1.0
    ratios = DR.check_bind(DR.bind_ref(means, parts, idx), w, p, rest, flags)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # max_distance = +inf switches the test off: only select and the non-finite means are left out
    (c, ok_c) = bind_raw(D, means, parts, select, math.inf)
    assert ok_c and np.array_equal(c[4] & 1, ((select == 0) | ~np.isfinite(means).all(1)).astype(np.uint8))
    # fewer than 8 finite particles: nobody is bound
    few = np.full((m, 3), np.nan, np.float32)
    few[[3, T + 2, 5, 7, 11, 13, m - 2]] = parts[[3, T + 2, 5, 7, 11, 13, m - 2]]
    (d, ok_d) = bind_raw(D, means, few)
    assert ok_d and (d[4] == DR.FLAG_UNBOUND).all() and (d[0] == -1).all() and not d[1].any() and not d[3].any()
    # the convenience wrapper gives the same bytes and counts the bound Gaussians
    bnd = D.bind_particles(_t(means), _t(parts), select=_t(select, np.uint8) != 0, max_distance=md)
    assert bnd.idx.cpu().numpy().tobytes() == idx.tobytes() and bnd.rest.cpu().numpy().tobytes() == rest.tobytes()
    assert bnd.n_bound() == int((~unbound).sum()) and (bnd.n, bnd.m) == (n, m)
    assert torch.equal(bnd.particles.isnan(), _t(parts).isnan())


# ---- 4. the apply ----------------------------------------------------------------------------------------------------------
def apply_raw(D, tensors, binding, mode, now, with_status=True):
    n = binding.n
    om, gm = guarded((n, 3), torch.float32)
    oq, gq = guarded((n, 4), torch.float32)
    osc, gs = guarded((n, 3), torch.float32)
    st, gst = guarded((n,), torch.uint8) if with_status else (None, None)
    D.deform_apply_raw(tensors["means"], tensors["quats"], tensors["scales"], binding, mode, now, om, oq, osc, status=st)
    torch.cuda.synchronize()
    ok = intact(gm, gq, gs) and (gst is None or intact(gst))
    return om.cpu().numpy(), oq.cpu().numpy(), osc.cpu().numpy(), (st.cpu().numpy() if with_status else None), ok


def scene(n, m, seed, kind="cloud"):
    mu, q, s, X = DR.cloud(n, m, seed, kind)
    return mu, q, s, X, dict(means=_t(mu), quats=_t(q), scales=_t(s), opacities=torch.full((n,), 0.5, device=DEV),
                             colors=torch.rand(n, 1, 3, device=DEV), sh_degree=0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_apply_against_fp64(D, n, mode):
    m = 700
    mu, q, s, X, tensors = scene(n, m, 10 * n + mode)
    select = np.ones(n, np.uint8)
    select[3::7] = 0                                                     # unbound rows (none when n = 1)
    arrays, ok = bind_raw(D, mu, X, select)
    assert ok
    binding = binding_of(D, arrays, m)
    idx, flags = arrays[0], arrays[4]
    worst = {}
    for motion in ("rigid", "bend", "stretch"):
        Y = DR.move(X, motion, seed=n)
        victim = int(idx[2, 0])                                          # a neighbour of Gaussian 0 blows up at frame time
        Y[victim] = (np.nan, np.inf)[mode], 0.0, 0.0
        now = _t(Y)
        om, oq, osc, st, ok = apply_raw(D, tensors, binding, mode, now)
        om2, oq2, osc2, st2, ok2 = apply_raw(D, tensors, binding, mode, now, with_status=False)
        assert ok and ok2 and st2 is None
        assert om.tobytes() == om2.tobytes() and oq.tobytes() == oq2.tobytes() and osc.tobytes() == osc2.tobytes()
        ref = DR.apply_ref(mu, q, s, *arrays, mode, Y, status_seen=st)
        hit = (idx == victim).any(0) & (flags & 1 == 0)
        assert hit[0] and (st[hit] == DR.ST_NONFINITE).all() and (st[flags & 1 != 0] == DR.ST_UNBOUND).all()
        assert np.isfinite(om).all()
        ratios = DR.check_apply(ref, mu, q, s, om, oq, osc, st)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(v <= 1.0 for v in ratios.values()), (motion, ratios)
        if n >= 63:
            assert (ref["branch"] == (2 if mode == 0 else 3)).sum() > n // 2
    print(f"\napply n {n} mode {mode}: worst ratios {worst}")


@pytest.mark.parametrize("kind", ["sheet", "strand", "collapsed"])
def test_apply_on_degenerate_neighbourhoods(D, kind):
    n, m = 300, 500
    mu, q, s, X, tensors = scene(n, m, 77, "cloud" if kind == "collapsed" else kind)
    arrays, ok = bind_raw(D, mu, X)
    binding = binding_of(D, arrays, m)
    for mode in (0, 1):
        Y = np.tile(np.float32([[0.25, -1.5, 3.0]]), (m, 1)) if kind == "collapsed" else DR.move(X, "bend")
        om, oq, osc, st, ok = apply_raw(D, tensors, binding, mode, _t(Y))
        assert ok
        ref = DR.apply_ref(mu, q, s, *arrays, mode, Y, status_seen=st)
        ratios = DR.check_apply(ref, mu, q, s, om, oq, osc, st)
        print(f"\n{kind} mode {mode}: ratios {ratios}, status {np.bincount(st, minlength=9).tolist()}")
        assert all(v <= 1.0 for v in ratios.values()), ratios
        if kind == "sheet":                                              # cloth: the rotation still, the affine mode falls back
            assert (st == (0 if mode == 0 else DR.ST_FALLBACK)).all() and "rot" in ratios
            assert osc.tobytes() == s.tobytes()
        else:                                                            # a strand, or a collapse at frame time: translated only
            assert (st == DR.ST_THIN).all()
            assert oq.tobytes() == q.tobytes() and osc.tobytes() == s.tobytes()
        if kind == "collapsed":
            assert np.abs(om - (Y[0] + arrays[3][0:3].T)).max() <= 4e-7 * 3.0


def test_deform_gaussians_contract(D):
    n, m = 500, 600
    mu, q, s, X, tensors = scene(n, m, 3)
    binding = D.bind_particles(tensors["means"], _t(X))
    now = _t(DR.move(X, "bend"))
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)
    a = D.deform_gaussians(tensors, binding, now, mode="affine", status=status)
    assert a["opacities"] is tensors["opacities"] and a["colors"] is tensors["colors"] and a["sh_degree"] == 0
    assert torch.equal(tensors["means"], _t(mu)) and torch.equal(tensors["scales"], _t(s))          # the rest state survives
    b = D.deform_gaussians(tensors, binding, now, mode="affine", out=a)
    assert all(b[k].data_ptr() == a[k].data_ptr() for k in ("means", "quats", "scales"))
    raw = apply_raw(D, tensors, binding, 1, now)
    assert b["means"].cpu().numpy().tobytes() == raw[0].tobytes() and b["scales"].cpu().numpy().tobytes() == raw[2].tobytes()
    assert status.cpu().numpy().tobytes() == raw[3].tobytes()
    with pytest.raises(ValueError, match="out is tensors"):
        D.deform_gaussians(tensors, binding, now, out=tensors)
    with pytest.raises(ValueError, match="rest state"):
        D.deform_gaussians(tensors, binding, now, out=dict(means=tensors["means"]))
    # a permuted scene with the permuted binding gives the permuted result, bit for bit
    order = torch.randperm(n, device=DEV)
    tp = {k: (v.index_select(0, order).contiguous() if torch.is_tensor(v) else v) for k, v in tensors.items()}
    c = D.deform_gaussians(tp, binding.reordered(order), now, mode="affine")
    for k in ("means", "quats", "scales"):
        assert torch.equal(c[k], b[k].index_select(0, order)), k


def test_an_empty_scene_deforms_to_an_empty_scene(D):
    """No Gaussian: every zero-element tensor has the same (null) address, which is no aliasing of the rest state."""
    _, _, _, X, tensors = scene(8, 40, 5)
    empty = {k: (v[:0].contiguous() if torch.is_tensor(v) else v) for k, v in tensors.items()}
    binding = D.bind_particles(empty["means"], _t(X))
    assert binding.n == 0 and binding.m == 40
    for mode in ("rigid", "affine"):
        out = D.deform_gaussians(empty, binding, _t(DR.move(X, "bend")), mode=mode)
        assert [tuple(out[k].shape) for k in ("means", "quats", "scales")] == [(0, 3), (0, 4), (0, 3)]
        assert out["colors"] is empty["colors"] and out["opacities"] is empty["opacities"]


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rigid", "affine"])
def test_apply_replays_in_a_graph(D, mode):
    n, m = 1000, 800
    mu, q, s, X, tensors = scene(n, m, 21)
    binding = D.bind_particles(tensors["means"], _t(X))
    frames = [_t(DR.move(X, motion, seed=k)) for k, motion in enumerate(("rigid", "bend", "stretch"))]
    eager = []
    for f in frames:
        st = torch.zeros(n, dtype=torch.uint8, device=DEV)
        o = D.deform_gaussians(tensors, binding, f, mode=mode, status=st)
        eager.append([o[k].clone() for k in ("means", "quats", "scales")] + [st])
    assert not torch.equal(eager[0][0], eager[1][0])
    now = frames[0].clone()
    out = {k: torch.empty_like(tensors[k]) for k in ("means", "quats", "scales")}
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        D.deform_gaussians(tensors, binding, now, mode=mode, out=out, status=st)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            D.deform_gaussians(tensors, binding, now, mode=mode, out=out, status=st)
        for k in (1, 2, 0):
            now.copy_(frames[k])
            for v in out.values():
                v.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for got, want in zip((out["means"], out["quats"], out["scales"], st), eager[k]):
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), k
    torch.cuda.synchronize()


# ---- 6. FrameRenderer(deform=) -----------------------------------------------------------------------------------------------
def cloth_scene(n_side=18, m_side=12):
    """A sheet of n_side^2 Gaussians over a grid of m_side^2 particles in front of a 64 x 64 camera, plus a rigid block."""
    rng = np.random.default_rng(8)
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, n_side), np.linspace(-0.8, 0.8, n_side), indexing="ij")
    sheet = np.stack([gx.reshape(-1), gy.reshape(-1), 0.01 * rng.normal(size=n_side * n_side)], 1)
    block = rng.uniform(-0.15, 0.15, (60, 3)) + [0.0, 0.0, 0.6]
    means = np.concatenate([sheet, block]).astype(np.float32)
    n = len(means)
    px, py = np.meshgrid(np.linspace(-0.9, 0.9, m_side), np.linspace(-0.9, 0.9, m_side), indexing="ij")
    parts = np.stack([px.reshape(-1), py.reshape(-1), np.zeros(m_side * m_side)], 1).astype(np.float32)
    quats = rng.normal(size=(n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    tensors = dict(means=_t(means), quats=_t(quats), scales=_t(np.exp(rng.uniform(-3.2, -2.6, (n, 3)))),
                   opacities=_t(rng.uniform(0.3, 0.9, n)), colors=_t(rng.uniform(0, 1, (n, 1, 3))), sh_degree=0)
    soft = np.arange(n) < n_side * n_side
    vm = np.eye(4, dtype=np.float32)
    vm[2, 3] = 2.5
    K = np.array([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]], np.float32)
    return tensors, parts, soft, vm, K


def wave(parts, phase):
    out = parts.copy()
    out[:, 2] = 0.15 * np.sin(3.0 * parts[:, 0] + phase)
    return out


def test_frame_renderer_deforms_per_frame(D):
    from robosimgs_amd import FrameRenderer, rasterization, transform_gaussians
    tensors, parts, soft, vm, K = cloth_scene()
    n = tensors["means"].shape[0]
    binding = D.bind_particles(tensors["means"], _t(parts), select=_t(soft, np.uint8))
    assert binding.n_bound() == int(soft.sum())
    r = FrameRenderer(tensors, 64, 64, render_mode="RGB+ED", frames_in_flight=2, isect_capacity=200_000, deform=binding,
                      deform_mode="rigid")
    assert r.order is not None and torch.equal(r.deform.flags, binding.flags.index_select(0, r.order))

    def by_hand(x, group_pose=None, renderer=r):
        posed = D.deform_gaussians(renderer.t, renderer.deform, _t(x), mode=renderer.deform_mode)
        if group_pose is not None:
            posed = transform_gaussians(posed, *group_pose, group_ids=renderer.group_ids, rotate_sh=False)
        return rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                             _t(vm)[None], _t(K)[None], 64, 64, sh_degree=0, render_mode="RGB+ED")

    def frame(tk, renderer=r):
        f = renderer.fetch(tk)
        got = f["colors"].clone(), f["alphas"].clone(), f["deform_status"].clone()
        renderer.release(tk)
        return got

    # the first frame of each slot shows the rest positions; particles on the host, on the device, as an array
    rest_c, rest_a, _ = by_hand(parts)
    c, a, st = frame(r.submit(vm, K))
    assert torch.equal(c, rest_c[0]) and torch.equal(a, rest_a[0]) and float(a.max()) > 0.5
    assert torch.equal(st != 0, (r.deform.flags & 1) != 0)                # cloth: rigid mode, nobody falls back
    frames = [wave(parts, 0.7 * k) for k in range(1, 5)]
    feeds = [frames[0], torch.from_numpy(frames[1]), _t(frames[2]), torch.from_numpy(frames[3]).double()]
    tickets = [r.submit(vm, K, particles=feeds[0]), r.submit(vm, K, particles=feeds[1])]
    got = [frame(tickets[0])]
    tickets.append(r.submit(vm, K, particles=feeds[2]))
    got.append(frame(tickets[1]))
    tickets.append(r.submit(vm, K, particles=feeds[3]))
    got += [frame(tickets[2]), frame(tickets[3])]
    for (c, a, _), x in zip(got, frames):
        wc, wa, _ = by_hand(x)
        assert torch.equal(c, wc[0]) and torch.equal(a, wa[0])
    assert not torch.equal(got[0][0], rest_c[0])
    # a submit without particles repeats the slot's previous deformation (two slots: frames[2], then frames[3])
    for x in (frames[2], frames[3]):
        c, a, _ = frame(r.submit(vm, K))
        wc, wa, _ = by_hand(x)
        assert torch.equal(c, wc[0]) and torch.equal(a, wa[0])
    # particles that the current stream is still writing when submit() is called: the slot's copy waits for them
    x, src = _t(frames[0]), _t(frames[1])
    torch.cuda._sleep(5_000_000)                                          # a couple of milliseconds ahead of the write
    x.copy_(src, non_blocking=True)
    c, a, _ = frame(r.submit(vm, K, particles=x))
    wc, wa, _ = by_hand(frames[1])
    assert torch.equal(c, wc[0]) and torch.equal(a, wa[0])
    c, a, _ = frame(r.submit(vm, K, particles=frames[2]))                 # (both slots hold frames[2] / frames[3] again)
    c, a, _ = frame(r.submit(vm, K, particles=frames[3]))
    # the renderer's permuted binding is the caller's, Gaussian by Gaussian
    mine = D.deform_gaussians(tensors, binding, _t(frames[0]))
    theirs = D.deform_gaussians(r.t, r.deform, _t(frames[0]))
    assert torch.equal(theirs["means"], mine["means"].index_select(0, r.order))
    # a wrong shape raises before any copy and leaves the slot free
    with pytest.raises(ValueError, match=r"particles must be \[144,3\]"):
        r.submit(vm, K, particles=frames[0][:-1])
    c, a, _ = frame(r.submit(vm, K))
    assert torch.equal(c, by_hand(frames[2])[0][0])

    # deform and group_ids on disjoint Gaussians: both are posed
    gid = torch.where(_t(soft, np.uint8) != 0, -1, 0).to(torch.int32)
    both = FrameRenderer(tensors, 64, 64, render_mode="RGB+ED", frames_in_flight=1, isect_capacity=200_000, deform=binding,
                         deform_mode="affine", group_ids=gid, n_groups=1, rotate_sh=False)
    ang = 0.6
    Rz = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1.0]])
    pose = ([Rz], [[0.2, -0.1, 0.0]])
    c, a, st = frame(both.submit(vm, K, rotations=pose[0], translations=pose[1], particles=frames[1]), both)
    wc, wa, _ = by_hand(frames[1], pose, both)
    assert torch.equal(c, wc[0]) and torch.equal(a, wa[0])
    assert not torch.equal(c, by_hand(frames[1], None, both)[0][0]) and not torch.equal(c, by_hand(parts, pose, both)[0][0])
    assert bool(((st & DR.ST_FALLBACK) != 0).any())                       # cloth in the affine mode falls back to rigid

    # construction errors
    with pytest.raises(ValueError, match="both bound to particles and in a group"):
        FrameRenderer(tensors, 64, 64, isect_capacity=200_000, deform=binding, group_ids=torch.zeros(n, dtype=torch.int32, device=DEV),
                      n_groups=1)
    with pytest.raises(ValueError, match="raw_params=True is not available with deform"):
        FrameRenderer(tensors, 64, 64, isect_capacity=200_000, deform=binding, raw_params=True)
    with pytest.raises(ValueError, match="deform_mode"):
        FrameRenderer(tensors, 64, 64, isect_capacity=200_000, deform=binding, deform_mode="elastic")
    with pytest.raises(ValueError, match="ParticleBinding"):
        FrameRenderer(tensors, 64, 64, isect_capacity=200_000, deform=binding.reordered(torch.arange(n - 1, device=DEV)))
    static = FrameRenderer(tensors, 64, 64, frames_in_flight=1, isect_capacity=200_000)
    with pytest.raises(ValueError, match="without deform"):
        static.submit(vm, K, particles=parts)
