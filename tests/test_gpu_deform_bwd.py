"""mgs_deform_apply_bwd on the GPU (include/mgs_deform_bwd.h, csrc/deform.hip) against the fp64 statement and the counted
bounds of tests/deform_bwd_ref.py: every gradient within its bound, bit-identity where the header promises it, the scatter's
edges, degenerate and inverted neighbourhoods, determinism, graph replay and the autograd plumbing.  The binding, the
forward's status and the cotangents are the GPU's own arrays: the statement is held on what the kernel read.
"""
import numpy as np
import pytest
import torch

import deform_ref as DR
import deform_bwd_ref as BR

pytestmark = pytest.mark.gpu
DEV = "cuda"
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
    buf = torch.full((nbytes + 16 + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf[:nbytes].view(dtype).view(shape), buf[nbytes:]


def intact(*guards):
    return all(bool((g == 0xA5).all().item()) for g in guards)


def bound_scene(D, n, m, seed, kind="cloud", unbound=True):
    """A scene bound on the GPU: numpy (q, X, arrays = idx, w, p, rest, flags), the binding and the device tensors."""
    mu, q, s, X = BR.lattice() if kind == "lattice" else DR.cloud(n, m, seed, kind)
    n = len(mu)
    select = np.ones(n, np.uint8)
    if unbound:
        select[3::7] = 0                                                    # unbound rows (none when n = 1)
    tensors = dict(means=_t(mu), quats=_t(q), scales=_t(s))
    binding = D.bind_particles(tensors["means"], _t(X), select=_t(select, np.uint8))
    arrays = [a.cpu().numpy() for a in (binding.idx, binding.w, binding.p, binding.rest, binding.flags)]
    return q, X, arrays, binding, tensors


def forward_status(D, tensors, binding, now):
    n = binding.n
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    D.deform_apply_raw(tensors["means"], tensors["quats"], tensors["scales"], binding, 0, now, torch.empty(n, 3, device=DEV),
                       torch.empty(n, 4, device=DEV), torch.empty(n, 3, device=DEV), status=st)
    return st


def bwd_raw(D, tensors, binding, now, status, ct, rest=True, with_bst=True, fill=0xA5):
    """mgs_deform_apply_bwd into guarded outputs with a workspace filled with `fill`: dict of numpy results (contrib is the
    workspace [8,3,n]) and whether every guard stayed intact."""
    n, m = binding.n, binding.m
    outs = {"v_particles": guarded((m, 3), torch.float32)}
    if rest:
        outs.update(v_means=guarded((n, 3), torch.float32), v_quats=guarded((n, 4), torch.float32),
                    v_scales=guarded((n, 3), torch.float32))
    bst, gb = guarded((n,), torch.uint8) if with_bst else (None, None)
    need = D.apply_bwd_workspace_bytes(n)
    ws = torch.full((need + 256 + GUARD,), fill, dtype=torch.uint8, device=DEV)
    pad = -ws.data_ptr() % 256
    tail = ws[pad + need:].clone()
    cts = [None if c is None else _t(c) for c in ct]
    D.deform_apply_bwd_raw(tensors["quats"], binding, now, status, *cts, rest=rest, out={k: v[0] for k, v in outs.items()},
                           bwd_status=bst, workspace=ws[:pad + need])
    torch.cuda.synchronize()
    ok = intact(*[v[1] for v in outs.values()]) and (gb is None or intact(gb)) and torch.equal(ws[pad + need:], tail)
    got = {k: v[0].cpu().numpy() for k, v in outs.items()}
    got["contrib"] = ws[pad:pad + 96 * n].view(torch.float32).view(DR.K, 3, n).cpu().numpy()
    got["bwd_status"] = bst.cpu().numpy() if with_bst else None
    got["idx"] = binding.idx.cpu().numpy()
    return got, ok


def held(D, q, arrays, binding, tensors, Y, ct, **kw):
    """One backward on the GPU held to the statement: (got, ref, ratios)."""
    now = _t(Y)
    status = forward_status(D, tensors, binding, now)
    got, ok = bwd_raw(D, tensors, binding, now, status, ct, **kw)
    assert ok, "a guard behind an output or the workspace was overwritten"
    ref = BR.bwd_ref(q, *arrays, Y, status.cpu().numpy(), *ct, guard_seen=got["bwd_status"])
    vp_ref, cnt = BR.scatter_ref(ref["contrib"], arrays[0], binding.m)
    ratios = BR.check_bwd(ref, vp_ref, got, *ct)
    return got, ref, ratios, cnt, status


def same_bytes(a, b, keys=("v_particles", "v_means", "v_quats", "v_scales", "contrib")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys if a.get(k) is not None and b.get(k) is not None)


# ---- 1. against fp64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_backward_against_fp64(D, n):
    """Worst error / bound measured on the MI355X (all n, all motions): see profiles/deform_bwd/README.md."""
    m = max(64, 3 * n)
    q, X, arrays, binding, tensors = bound_scene(D, n, m, 10 * n)
    idx, flags = arrays[0], arrays[4]
    ct = BR.cotangents(n, n)
    worst = {}
    for motion in ("rigid", "bend", "stretch"):
        Y = DR.move(X, motion, seed=n)
        victim = int(idx[2, 0])                                            # a neighbour of Gaussian 0 blows up at frame time
        Y[victim] = np.nan, 0.0, 0.0
        got, ref, ratios, cnt, status = held(D, q, arrays, binding, tensors, Y, ct)
        st = status.cpu().numpy()
        hit = (idx == victim).any(0) & (flags & 1 == 0)
        assert hit[0] and (st[hit] == DR.ST_NONFINITE).all() and (ref["kind"][hit] == 0).all()
        assert (ref["kind"][flags & 1 != 0] == 0).all() and not got["bwd_status"].any()
        assert not got["v_particles"][victim].any()                        # every row that touches it passes through
        assert np.isfinite(got["v_particles"]).all() and np.isfinite(got["v_means"]).all()
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(v <= 1.0 for v in ratios.values()), (motion, ratios)
        if n >= 63:
            assert (ref["kind"] == 2).sum() > n // 2
        if motion == "bend":
            # bits: a second run, no bwd_status, a zeroed workspace, no rest gradients, and single null cotangents
            now = _t(Y)
            for kw in (dict(), dict(with_bst=False), dict(fill=0), dict(rest=False)):
                again, ok = bwd_raw(D, tensors, binding, now, status, ct, **kw)
                assert ok and same_bytes(got, again), kw
            g0, ref0, r0, _, _ = held(D, q, arrays, binding, tensors, Y, (ct[0], None, None))
            assert all(v <= 1.0 for v in r0.values()), r0
            assert not g0["v_quats"][ref0["kind"] <= 1].any() and not g0["v_scales"].any()
    print(f"\nbackward n {n}: worst ratios {({k: round(v, 4) for k, v in worst.items()})}")


# ---- 2. the scatter's edges ---------------------------------------------------------------------------------------------
def test_scatter_with_segments_far_longer_than_a_wave(D):
    n, m = 4097, 8
    q, X, arrays, binding, tensors = bound_scene(D, n, m, 5, unbound=False)
    ct = BR.cotangents(n, 2)
    got, ref, ratios, cnt, _ = held(D, q, arrays, binding, tensors, DR.move(X, "bend"), ct)
    assert (cnt == n).all()                                                 # every particle is every Gaussian's neighbour
    t_start, t_entry = binding.transposed()
    assert t_start.cpu().tolist() == [n * j for j in range(m + 1)]
    print(f"\nscatter n {n} m {m}: ratios {({k: round(v, 4) for k, v in ratios.items()})}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the kernel's order of additions, bit for bit: the lanes' chains and the xor tree of the header on the GPU's own fp32
    # contributions
    flat = got["contrib"].transpose(1, 0, 2).reshape(3, DR.K * n)
    ts, te = t_start.cpu().numpy(), t_entry.cpu().numpy()
    for j in range(m):
        ent = te[ts[j]:ts[j + 1]]
        lanes = np.zeros((3, 64), np.float32)
        for r in range(0, len(ent), 64):
            chunk = flat[:, ent[r:r + 64]]
            lanes[:, :chunk.shape[1]] = lanes[:, :chunk.shape[1]] + chunk
        for d in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, np.arange(64) ^ d]
        assert lanes[:, 0].tobytes() == got["v_particles"][j].tobytes(), j


def test_scatter_leaves_exact_zeros_for_unreferenced_particles(D):
    n, m = 1, 64
    q, X, arrays, binding, tensors = bound_scene(D, n, m, 6, unbound=False)
    ct = BR.cotangents(n, 3)
    got, ref, ratios, cnt, _ = held(D, q, arrays, binding, tensors, DR.move(X, "bend"), ct)
    assert (cnt == 0).sum() == 56 and (ref["kind"] == 2).all()
    assert got["v_particles"][cnt == 0].tobytes() == bytes(56 * 12)         # +0, every bit
    assert got["v_particles"][cnt > 0].all()
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ---- 3. degenerate and inverted neighbourhoods ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sheet", "strand", "collapsed", "mirrored", "mirrored_lattice"])
def test_backward_on_degenerate_neighbourhoods(D, kind):
    """mirrored: a random volume reflected at frame time, det P < 0 everywhere, no row near the guard (the smallest
    (sigma_2 - sigma_3) / sigma_1 is 4e-3).  mirrored_lattice: sigma_2 = sigma_3 to rounding, every row guarded."""
    n, m = {"mirrored": (4097, 3 * 4097), "mirrored_lattice": (27, 125)}.get(kind, (300, 500))
    shape = {"collapsed": "cloud", "mirrored": "cloud", "mirrored_lattice": "lattice"}.get(kind, kind)
    q, X, arrays, binding, tensors = bound_scene(D, n, m, 77, shape, unbound=kind != "mirrored_lattice")
    ct = BR.cotangents(n, 4)
    if kind == "collapsed":
        Y = np.tile(np.float32([[0.25, -1.5, 3.0]]), (m, 1))
    else:
        Y = DR.move(X, "rigid" if kind == "mirrored_lattice" else "bend")
        if kind.startswith("mirrored"):
            Y = BR.mirror(Y)
    got, ref, ratios, cnt, status = held(D, q, arrays, binding, tensors, Y, ct)
    bound = ref["kind"] > 0
    print(f"\n{kind}: rows pass-through, thin, turned {np.bincount(ref['kind'], minlength=3).tolist()}, guarded "
          f"{int(ref['guard'].sum())}, free {int(ref['free'].sum())}, ratios {({k: round(v, 4) for k, v in ratios.items()})}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if kind == "sheet":                                                     # cloth: every bound row turns
        assert (ref["kind"][bound] == 2).all() and not got["bwd_status"].any()
    elif kind in ("strand", "collapsed"):                                   # translated only: the particle part comes from c alone
        assert (ref["kind"][bound] == 1).all() and not got["bwd_status"].any()
        w = arrays[1].astype(np.float64)
        want = (w[1:, None, :] * ct[0].astype(np.float64).T[None]).astype(np.float32)
        assert got["contrib"][1:][:, :, bound].tobytes() == want[:, :, bound].tobytes()
    else:                                                                   # det P < 0 everywhere
        e = Y[arrays[0]].astype(np.float64)
        P = np.einsum("kna,knb->nab", (e[1:] - e[0])[:, bound], np.transpose(arrays[2].astype(np.float64), (0, 2, 1))[1:][:, bound])
        assert (np.linalg.det(P) < 0).all() and (ref["kind"][bound] == 2).all()
        assert (ref["ratio"][bound] < 1.0).all()
        gd = got["bwd_status"] != 0
        assert not gd[~bound].any() and (ref["ratio"][gd] < 2e-3).all()
        assert gd.all() if kind == "mirrored_lattice" else (ref["kind"] == 2).sum() - gd.sum() > n // 2
        # a guarded row's particle part is the thin row's
        if gd.any():
            w = arrays[1].astype(np.float64)
            want = (w[1:, None, :] * ct[0].astype(np.float64).T[None]).astype(np.float32)
            assert got["contrib"][1:][:, :, gd].tobytes() == want[:, :, gd].tobytes()
            assert got["v_quats"][gd].tobytes() == ct[1][gd].tobytes()


# ---- 4. graph capture ---------------------------------------------------------------------------------------------------
def test_backward_replays_in_a_graph(D):
    n, m = 1000, 800
    q, X, arrays, binding, tensors = bound_scene(D, n, m, 21)
    frames = [_t(DR.move(X, motion, seed=k)) for k, motion in enumerate(("rigid", "bend", "stretch"))]
    cts = [[_t(c) for c in BR.cotangents(n, 30 + k)] for k in range(3)]
    binding.transposed()                                                    # built outside the capture
    ws = torch.empty(D.apply_bwd_workspace_bytes(n) + 256, dtype=torch.uint8, device=DEV)
    names = ("v_particles", "v_means", "v_quats", "v_scales")
    eager = []
    for f, ct in zip(frames, cts):
        st = forward_status(D, tensors, binding, f)
        bst = torch.zeros(n, dtype=torch.uint8, device=DEV)
        res = D.deform_apply_bwd_raw(tensors["quats"], binding, f, st, *ct, bwd_status=bst)
        eager.append([res[k].clone() for k in names] + [bst, st])
    assert not torch.equal(eager[0][0], eager[1][0])
    now, ct, st = frames[0].clone(), [c.clone() for c in cts[0]], eager[0][5].clone()
    out = {"v_particles": torch.empty(m, 3, device=DEV), "v_means": torch.empty(n, 3, device=DEV),
           "v_quats": torch.empty(n, 4, device=DEV), "v_scales": torch.empty(n, 3, device=DEV)}
    bst = torch.zeros(n, dtype=torch.uint8, device=DEV)
    call = lambda: D.deform_apply_bwd_raw(tensors["quats"], binding, now, st, *ct, out=out, bwd_status=bst, workspace=ws)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call()
        for k in (1, 2, 0):
            now.copy_(frames[k])
            st.copy_(eager[k][5])
            for dst, src in zip(ct, cts[k]):
                dst.copy_(src)
            for v in out.values():
                v.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for got, want in zip([out[key] for key in names] + [bst], eager[k]):
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), k
    torch.cuda.synchronize()


# ---- 5. the autograd plumbing -------------------------------------------------------------------------------------------
def test_autograd_through_the_renderer(D):
    from robosimgs_amd import rasterization
    from test_gpu_deform import cloth_scene, wave
    tensors, parts, soft, vm, K = cloth_scene()
    n = tensors["means"].shape[0]
    binding = D.bind_particles(tensors["means"], _t(parts), select=_t(soft, np.uint8))
    x = _t(wave(parts, 0.7)).requires_grad_(True)
    leaves = {k: tensors[k].clone().requires_grad_(True) for k in ("means", "quats", "scales")}
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)
    posed = D.deform_gaussians_autograd(dict(tensors, **leaves), binding, x, status=status)
    assert posed["opacities"] is tensors["opacities"] and posed["colors"] is tensors["colors"] and posed["sh_degree"] == 0
    for k in ("means", "quats", "scales"):
        assert posed[k].requires_grad
        posed[k].retain_grad()
    plain = D.deform_gaussians(tensors, binding, x.detach())
    assert all(torch.equal(plain[k], posed[k].detach()) and not plain[k].requires_grad for k in ("means", "quats", "scales"))
    colors, alphas, _ = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                      _t(vm)[None], _t(K)[None], 64, 64, sh_degree=0)
    weight = torch.linspace(0.5, 1.5, 64 * 64 * 3, device=DEV).reshape(1, 64, 64, 3)
    ((colors * weight).sum() + alphas.sum()).backward()
    ct = [posed[k].grad.contiguous() for k in ("means", "quats", "scales")]
    assert all(c is not None and bool(c.abs().sum() > 0) for c in ct[:1])
    raw = D.deform_apply_bwd_raw(tensors["quats"], binding, x.detach(), status, *ct)
    assert x.grad.cpu().numpy().tobytes() == raw["v_particles"].cpu().numpy().tobytes() and bool(x.grad.abs().sum() > 0)
    for k, name in (("means", "v_means"), ("quats", "v_quats"), ("scales", "v_scales")):
        assert leaves[k].grad.cpu().numpy().tobytes() == raw[name].cpu().numpy().tobytes(), k
    # only the particles ask for a gradient: the same bits, and no rest gradients are made
    x2 = x.detach().clone().requires_grad_(True)
    posed2 = D.deform_gaussians_autograd(tensors, binding, x2)
    c2, a2, _ = rasterization(posed2["means"], posed2["quats"], posed2["scales"], posed2["opacities"], posed2["colors"],
                              _t(vm)[None], _t(K)[None], 64, 64, sh_degree=0)
    ((c2 * weight).sum() + a2.sum()).backward()
    assert torch.equal(x2.grad, x.grad)
    with pytest.raises(NotImplementedError):
        D.deform_gaussians_autograd(tensors, binding, x, mode="affine")
    with pytest.raises(NotImplementedError):
        D.deform_gaussians_autograd(dict(tensors, colors=torch.zeros(n, 4, 3, device=DEV), sh_degree=1), binding, x, rotate_sh=True)
    again = D.deform_gaussians(dict(tensors, **leaves), binding, x)
    assert all(not again[k].requires_grad and again[k].grad_fn is None for k in ("means", "quats", "scales"))
    # a trained mean takes effect through shift_offsets_: the bound rows move by R delta, the others not at all
    delta = torch.zeros(n, 3, device=DEV)
    delta[:, 2] = 0.01
    before = D.deform_gaussians(tensors, binding, x.detach())["means"].clone()
    binding.shift_offsets_(delta)
    after = D.deform_gaussians(tensors, binding, x.detach())["means"]
    moved = (after - before).norm(dim=1)
    sel = _t(soft, np.uint8) != 0
    assert bool((moved[~sel] == 0).all()) and bool(((moved[sel] - 0.01).abs() < 1e-5).all())
