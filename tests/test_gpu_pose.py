"""mgs_pose_bwd (csrc/pose.hip) and pose_gaussians on the GPU, held to the fp64 reference of tests/pose_ref.py under its
counted bounds: every path of the kernel, the group patterns a wave can hold, null cotangents, bit-reproducibility, guard
bands, and the link inside a real rendering backward -- each link judged in fp64 at the GPU's own inputs to that link.

Worst ratios to the bounds measured on an MI355X are recorded in profiles/pose/README.md; the gate is ratio <= 1.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import frame_helper_ref as FR
import pose_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
NAMES = ("v_means", "v_quats", "v_scales", "v_sh")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pattern(pattern, n, K):
    """(gids int32 [n] or None, n_groups, rotations, translations, scales) of a group pattern."""
    inp = FR.transform_inputs(n, K)
    three = (np.stack(inp["rotations"]), np.stack(inp["translations"]), np.array(inp["group_scales"]))
    if pattern == "mixed":                       # ids from TRANSFORM_GIDS with 3 groups: -1, 3 and 7 do not move
        return inp["gids"], 3, *three
    if pattern == "one":                         # group_ids null: all in group 0
        return None, 1, three[0][:1], three[1][:1], three[2][:1]
    if pattern == "rr70":                        # round-robin over 70 groups: every wave holds 64 different ids
        return (np.arange(n) % 70).astype(np.int32), 70, *PR.random_poses(70, seed=70)
    if pattern == "empty":                       # nobody is in group 1
        return np.where(inp["gids"] == 1, 2, inp["gids"]).astype(np.int32), 3, *three
    if pattern == "single_last":                 # group 3 owns one Gaussian, the last of the last, partial wave
        g = (np.arange(n) % 3).astype(np.int32)
        g[-1] = 3
        return g, 4, *PR.random_poses(4, seed=4)
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def _case(n, K, degree, pattern="mixed"):
    """Inputs of one backward: the forward run on the GPU (its posed outputs are what the backward reads), cotangents."""
    from robosimgs_amd.transform import pack_transforms, transform_gaussians
    inp = FR.transform_inputs(n, K)
    gids, G, R, t, s = _pattern(pattern, n, K)
    x, rot = pack_transforms(R, t, s, degree)
    tensors = {k: _t(inp[k]) for k in ("means", "quats", "scales", "opacities", "colors")}
    tensors["sh_degree"] = degree
    gd = _t(gids) if gids is not None else None
    xd, rd = _t(x), _t(rot)
    posed = transform_gaussians(tensors, group_ids=gd, packed=(xd, rd))
    assert posed["colors"].data_ptr() != tensors["colors"].data_ptr()
    ct = PR.cotangents(n, K)
    c = dict(n=n, K=K, degree=degree, G=G, gids=gids, gd=gd, x=x, rot=rot, xd=xd, rd=rd, ct=ct, ctd=[_t(a) for a in ct],
             posed=[posed[k] for k in ("means", "quats", "scales", "colors")])
    c["posed_np"] = [a.cpu().numpy() for a in c["posed"]]
    return c


def _buffers(c, sh, rest, guard=0, fill=0xA5):
    """v_pose and the rest-pose gradient buffers (uint8 storage, `guard` bytes of 0xA5 behind each)."""
    sizes = {"v_pose": c["G"] * 8 * 4}
    if rest:
        sizes.update(v_means=c["n"] * 12, v_quats=c["n"] * 16, v_scales=c["n"] * 12)
        if sh:
            sizes["v_sh"] = c["n"] * c["K"] * 12
    return {k: (torch.full((b + guard,), fill, dtype=torch.uint8, device=DEV), b) for k, b in sizes.items()}


def _call(c, which=(True, True, True, True), sh=True, rest=True, zeros=False, guard=0, workspace=None):
    """mgs_pose_bwd through ctypes.  which: the cotangents that are given (the others null, or explicit zero tensors with
    zeros=True).  Returns (dict of numpy results, dict of raw buffers, workspace tensor)."""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    L = _lib.lib()
    cts = [(d if w else (torch.zeros_like(d) if zeros else None)) for d, w in zip(c["ctd"], which)]
    if not sh:
        cts[3] = None
    bufs = _buffers(c, sh, rest, guard)
    need = L.mgs_pose_bwd_workspace_bytes(c["n"], c["G"])
    if workspace is None:
        workspace = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert workspace.data_ptr() % 256 == 0 and all(b.data_ptr() % 16 == 0 for b, _ in bufs.values())
    m, q, s, col = c["posed"]
    bp = lambda k: ptr(bufs[k][0]) if k in bufs else None
    check(L.mgs_pose_bwd(c["n"], ptr(m), ptr(q), ptr(s), c["degree"], c["K"], ptr(col) if sh else None, ptr(c["gd"]), c["G"],
                         ptr(c["xd"]), ptr(c["rd"]) if sh else None, ptr(cts[0]), ptr(cts[1]), ptr(cts[2]), ptr(cts[3]),
                         bp("v_means"), bp("v_quats"), bp("v_scales"), bp("v_sh"), bp("v_pose"), ptr(workspace), need,
                         stream_handle()), "mgs_pose_bwd")
    shapes = dict(v_pose=(c["G"], 8), v_means=(c["n"], 3), v_quats=(c["n"], 4), v_scales=(c["n"], 3), v_sh=(c["n"], c["K"], 3))
    out = {k: b[:nb].view(torch.float32).reshape(shapes[k]).cpu().numpy() for k, (b, nb) in bufs.items()}
    return out, bufs, workspace


@functools.lru_cache(maxsize=None)
def _ref(n, K, degree, pattern, which, sh):
    c = _case(n, K, degree, pattern)
    m, q, s, col = c["posed_np"]
    cts = [a if w else None for a, w in zip(c["ct"], which)]
    return PR.pose_ref(m, q, s, col if sh else None, degree, c["gids"], c["G"], c["x"], c["rot"], cts[0], cts[1], cts[2],
                       cts[3] if sh else None)


def _check(c, out, pattern="mixed", which=(True, True, True, True), sh=True, rest=True, tag=""):
    ref = _ref(c["n"], c["K"], c["degree"], pattern, tuple(which), sh)
    ratios = {}
    vp, bp = ref["v_pose"]
    assert not out["v_pose"][:, 7].any()
    for name, cols in (("omega", slice(0, 3)), ("t", slice(3, 6)), ("lambda", slice(6, 7))):
        ratios[name] = FR.worst_ratio(out["v_pose"][:, cols], vp[:, cols], bp[:, cols])
    if rest:
        for name in NAMES[:4 if sh else 3]:
            ratios[name] = FR.worst_ratio(out[name], *ref[name])
    else:
        assert set(out) == {"v_pose"}
    print(f"\n{tag} n {c['n']} K {c['K']} degree {c['degree']} {pattern} sh {sh} rest {rest}: worst ratio to the bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()), end="")
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- every path of the kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rest", [True, False])
@pytest.mark.parametrize("K,degree,sh", [(K, d, True) for K, d in FR.TRANSFORM_CASES] + [(16, 3, False)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_every_path_against_the_reference(n, K, degree, sh, rest):
    c = _case(n, K, degree)
    out, _b, _w = _call(c, sh=sh, rest=rest)
    _check(c, out, sh=sh, rest=rest, tag="paths")


# ---- group patterns -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["one", "mixed", "rr70", "empty", "single_last"])
def test_group_patterns(pattern):
    n, K, degree = 4097, 16, 3
    c = _case(n, K, degree, pattern)
    out, _b, _w = _call(c)
    _check(c, out, pattern, tag="groups")
    if pattern == "mixed":                       # -1, 3 and 7 do not move: their rows are the cotangent's bits
        still = ~np.isin(c["gids"], (0, 1, 2))
        assert still.sum() > n // 3
        for name, ct in zip(NAMES, c["ct"]):
            assert np.array_equal(_bits(out[name])[still], _bits(ct)[still]), name
        # and of the rows that move, the DC term is the cotangent's bits too
        assert np.array_equal(_bits(out["v_sh"])[:, 0], _bits(c["ct"][3])[:, 0])
    if pattern == "rr70":
        assert c["G"] == 70 and len(set(c["gids"][:64])) == 64
    if pattern == "empty":
        assert not (c["gids"] == 1).any() and not _bits(out["v_pose"])[1].any()          # all zero bits
        assert out["v_pose"][0].any() and out["v_pose"][2].any()
    if pattern == "single_last":
        assert (c["gids"] == 3).sum() == 1 and c["gids"][-1] == 3 and n % 64 == 1
        assert out["v_pose"][3, :7].all()


# ---- null cotangents ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alone", [0, 1, 2, 3])
def test_a_null_cotangent_is_a_zero_cotangent(alone):
    c = _case(4097, 16, 3)
    which = tuple(i == alone for i in range(4))
    null, _b, _w = _call(c, which=which)
    zero, _b, _w = _call(c, which=which, zeros=True)
    for k in null:
        assert np.array_equal(_bits(null[k]), _bits(zero[k])), k
    _check(c, null, which=which, tag="null")
    none, _b, _w = _call(c, which=(False,) * 4)
    assert not any(v.any() for v in none.values())                       # zero (of either sign) everywhere


# ---- same bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["mixed", "rr70"])
def test_two_calls_give_the_same_bits(pattern):
    c = _case(4097, 16, 3, pattern)
    first, _b, ws = _call(c)
    ws.fill_(0xA5)                                # nothing of the first call is left for the second
    second, _b, _w = _call(c, workspace=ws)
    third, _b, _w = _call(c, workspace=torch.zeros_like(ws))
    for k in first:
        assert np.array_equal(_bits(first[k]), _bits(second[k])) and np.array_equal(_bits(first[k]), _bits(third[k])), k


# ---- beyond a single trip of the second stage -----------------------------------------------------------------
def test_more_chunks_than_one_trip_of_the_last_stage():
    n = 300_001
    assert ((n + 63) // 64 + 63) // 64 > 64           # more chunks of 64 waves than the last stage's 64 lanes
    c = _case(n, 16, 3)
    out, _b, _w = _call(c)
    _check(c, out, tag="large")


# ---- guard bands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("K,degree", [(16, 3), (9, 2)])
def test_guard_bands_are_intact(n, K, degree):
    c = _case(n, K, degree)
    out, bufs, ws = _call(c, guard=GUARD)
    from robosimgs_amd import _lib
    need = _lib.lib().mgs_pose_bwd_workspace_bytes(n, c["G"])
    assert ws.numel() == need + GUARD and bool((ws[need:] == 0xA5).all())
    for k, (b, nb) in bufs.items():
        assert b.numel() == nb + GUARD and bool((b[nb:] == 0xA5).all()), k
    _check(c, out, tag="guard")


# ---- what autograd receives -----------------------------------------------------------------------------------
def test_pose_gaussians_hands_autograd_the_ambient_gradients():
    """v_R = 1/2 [v_omega]x R, v_t and v_s = v_lambda / s out of pose_gaussians' backward, with fp64 poses so that the
    chain after the kernel is exact: the bounds are the kernel's, carried through the (linear) chain."""
    from robosimgs_amd.pose import pack_transforms_torch, pose_gaussians
    n, K, degree = 4097, 16, 3
    inp = FR.transform_inputs(n, K)
    tensors = {k: _t(inp[k]).requires_grad_(k != "opacities") for k in ("means", "quats", "scales", "opacities", "colors")}
    tensors["sh_degree"] = degree
    R, t, s = (torch.tensor(np.stack(inp[k]), dtype=torch.float64, device=DEV, requires_grad=True)
               for k in ("rotations", "translations", "group_scales"))
    gids = _t(inp["gids"])
    posed = pose_gaussians(tensors, R, t, s, group_ids=gids)
    keys = ("means", "quats", "scales", "colors")
    cts = PR.cotangents(n, K)
    torch.autograd.backward([posed[k] for k in keys], [_t(c) for c in cts])
    x, rot = pack_transforms_torch(R, t, s, degree)
    f = lambda a: a.detach().cpu().numpy()
    ref = PR.pose_ref(*[f(posed[k]) for k in keys], degree, inp["gids"], 3, f(x), f(rot), *cts)
    vp, bp = ref["v_pose"]
    ratios = {name: FR.worst_ratio(f(tensors[k].grad), *ref[name]) for name, k in zip(NAMES, keys)}
    Rn, sn = f(R), f(s)
    for g in range(3):
        b = bp[g, 0:3]
        absskew = np.array([[0, b[2], b[1]], [b[2], 0, b[0]], [b[1], b[0], 0]])
        ratios[f"R{g}"] = FR.worst_ratio(f(R.grad)[g], PR.tangent_to_ambient(vp[g, 0:3], Rn[g]), 0.5 * absskew @ np.abs(Rn[g]))
    ratios["t"] = FR.worst_ratio(f(t.grad), vp[:, 3:6], bp[:, 3:6])
    ratios["s"] = FR.worst_ratio(f(s.grad), vp[:, 6] / sn, bp[:, 6] / sn)
    assert R.grad.dtype == t.grad.dtype == s.grad.dtype == torch.float64 and tensors["means"].grad.dtype == torch.float32
    print("\nautograd: worst ratio to the bound " + ", ".join(f"{k_} {v:.3f}" for k_, v in ratios.items()), end="")
    assert max(ratios.values()) <= 1.0, ratios
    # no SH rotation: the colours are the caller's tensor, and no gradient is made up for them
    tensors2 = {k: (v.detach().requires_grad_(k == "means") if torch.is_tensor(v) else v) for k, v in tensors.items()}
    posed2 = pose_gaussians(tensors2, R.detach(), t.detach(), group_ids=gids, rotate_sh=False)
    assert posed2["colors"] is tensors2["colors"] and posed2["opacities"] is tensors2["opacities"]
    posed2["means"].backward(_t(cts[0]))
    x2, rot2 = pack_transforms_torch(R, t, None, 0)
    assert rot2 is None
    ref2 = PR.pose_ref(*[f(posed2[k]) for k in keys[:3]], None, degree, inp["gids"], 3, f(x2), None, cts[0])
    assert FR.worst_ratio(f(tensors2["means"].grad), *ref2["v_means"]) <= 1.0


@pytest.mark.parametrize("used", [0, 1, 2, 3])
def test_an_unused_output_reaches_the_kernel_as_null(used, monkeypatch):
    """A loss that uses one posed output: autograd hands None for the other three, no zero tensor is made, mgs_pose_bwd gets
    NULL for them -- and every gradient has the bits that explicit zero cotangents give."""
    from robosimgs_amd import pose
    n, K, degree = 4097, 16, 3
    inp = FR.transform_inputs(n, K)
    keys = ("means", "quats", "scales", "colors")
    seen = []
    raw = pose.pose_bwd_raw

    def spy(*args, **kw):
        seen.append([a is not None for a in args[8:12]])
        return raw(*args, **kw)
    monkeypatch.setattr(pose, "pose_bwd_raw", spy)

    def run(explicit_zeros):
        tensors = {k: _t(inp[k]).requires_grad_(k in keys) for k in keys + ("opacities",)}
        tensors["sh_degree"] = degree
        R, t, s = (torch.tensor(np.stack(inp[k]), dtype=torch.float64, device=DEV, requires_grad=True)
                   for k in ("rotations", "translations", "group_scales"))
        posed = pose.pose_gaussians(tensors, R, t, s, group_ids=_t(inp["gids"]))
        ct = _t(PR.cotangents(n, K)[used])
        if explicit_zeros:
            torch.autograd.backward([posed[k] for k in keys], [ct if i == used else torch.zeros_like(posed[k])
                                                               for i, k in enumerate(keys)])
        else:
            (posed[keys[used]] * ct).sum().backward()
        return [tensors[k].grad for k in keys] + [R.grad, t.grad, s.grad]
    alone, zeros = run(False), run(True)
    assert seen == [[i == used for i in range(4)], [True] * 4]
    for a, z in zip(alone, zeros):
        assert a is not None and a.dtype == z.dtype and torch.equal(a.view(torch.uint8), z.view(torch.uint8))
    assert bool(alone[used].abs().sum() > 0) and any(bool(g.abs().sum() > 0) for g in alone[4:])   # (scales move v_lambda only)


def test_a_second_backward_through_the_pose_raises():
    from robosimgs_amd.pose import pose_gaussians
    inp = FR.transform_inputs(65, 4)
    tensors = {k: _t(inp[k]) for k in ("means", "quats", "scales", "opacities", "colors")}
    tensors["sh_degree"] = 1
    R, t = (torch.tensor(np.stack(inp[k]), dtype=torch.float64, device=DEV, requires_grad=True)
            for k in ("rotations", "translations"))
    posed = pose_gaussians(tensors, R, t, group_ids=_t(inp["gids"]))
    (g,) = torch.autograd.grad(posed["means"].sum(), t, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---- the link inside a real backward --------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _example():
    spec = importlib.util.spec_from_file_location("fit_joint_angle", os.path.join(ROOT, "examples", "fit_joint_angle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _lid_scene():
    from robosimgs_amd.articulation import Hinge
    E = _example()
    scene, ids, edge, axis = E.lid_scene()
    joint = np.zeros(16)
    joint[0:3], joint[3:6] = edge, axis
    cam = E.scene_camera(64, 64)
    cam_t = (_t(cam.viewmat()[None].astype(np.float32)), _t(cam.K[None].astype(np.float32)))
    return E, scene, ids, Hinge(joint), cam_t


def test_the_link_inside_a_rendering_backward():
    from robosimgs_amd import l1_loss, rasterization
    from robosimgs_amd.pose import pack_transforms_torch, pose_gaussians
    E, scene, ids, hinge, cam_t = _lid_scene()
    n = len(scene)
    assert 250 <= n <= 350 and scene.sh_degree == 3
    tensors = scene.to_torch(DEV, 3)
    leaves = ("means", "quats", "scales", "colors")
    for k in leaves:
        tensors[k].requires_grad_(True)
    gids = _t(np.where(ids == E.LID, 0, 1).astype(np.int32))                 # group 0 the lid, group 1 the body
    theta = torch.tensor(0.55, dtype=torch.float64, device=DEV, requires_grad=True)
    t_body = torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64, device=DEV, requires_grad=True)
    with torch.no_grad():
        target = E.render_posed(tensors, torch.where(gids == 0, 0, -1).to(torch.int32), hinge,
                                torch.tensor(E.THETA_STAR, dtype=torch.float64, device=DEV), cam_t, 64, 64)
    R, t = hinge.pose_torch(theta)
    rotations = torch.stack([R, torch.eye(3, dtype=torch.float64, device=DEV)])
    translations = torch.stack([t, t_body])
    posed = pose_gaussians(tensors, rotations, translations, group_ids=gids)
    for k in leaves:
        posed[k].retain_grad()
    colors, _a, _m = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                   cam_t[0], cam_t[1], 64, 64, sh_degree=3)
    l1_loss(colors, target).backward()
    cts = [posed[k].grad for k in leaves]
    assert all(g is not None and bool(g.abs().sum() > 0) for g in cts)
    x, rot = pack_transforms_torch(rotations, translations, None, 3)        # what the forward read
    f = lambda a: a.detach().cpu().numpy()
    ref = PR.pose_ref(f(posed["means"]), f(posed["quats"]), f(posed["scales"]), f(posed["colors"]), 3, f(gids), 2, f(x),
                      f(rot), *[f(g) for g in cts])
    ratios = {name: FR.worst_ratio(f(tensors[k].grad), *ref[name]) for name, k in zip(NAMES, leaves)}
    vp, bp = ref["v_pose"]
    ratios["t_body"] = FR.worst_ratio(f(t_body.grad), vp[1, 3:6], bp[1, 3:6])
    # theta through Rodrigues in fp64: dR/dtheta = [k]x R and dt/dtheta = -[k]x R p, so <v_R, dR> = v_omega . k
    k = hinge.axis / np.linalg.norm(hinge.axis)
    Rn, _tn = hinge.pose(float(theta.detach()))
    dt = -np.cross(k, Rn @ hinge.position)
    want = vp[0, 0:3] @ k + vp[0, 3:6] @ dt
    bound = bp[0, 0:3] @ np.abs(k) + bp[0, 3:6] @ np.abs(dt)
    ratios["theta"] = abs(float(theta.grad) - want) / bound
    print(f"\nlink: n {n}, theta.grad {float(theta.grad):+.6e} (fp64 {want:+.6e}, bound {bound:.2e}); worst ratio to the bound "
          + ", ".join(f"{k_} {v:.3f}" for k_, v in ratios.items()), end="")
    assert abs(want) > 100 * bound                                          # the gradient is not noise
    assert max(ratios.values()) <= 1.0, ratios


# ---- recovery -------------------------------------------------------------------------------------------------
def test_the_angle_of_the_lid_is_recovered():
    """The example's loop.  The fp64 torch oracle's loop (oracle/gs_oracle_torch.render under the same transform written
    in torch, on the CPU) reaches |theta_K - theta*| = 0.0017 |theta_0 - theta*| with these settings
    (profiles/pose/README.md has its trajectory): well under 1/16, so 1/4 is a condition with margin."""
    E, scene, ids, hinge, cam_t = _lid_scene()
    tensors = scene.to_torch(DEV, 3)
    gids = _t(np.where(ids == E.LID, 0, -1).astype(np.int32))
    with torch.no_grad():
        target = E.render_posed(tensors, gids, hinge, torch.tensor(E.THETA_STAR, dtype=torch.float64, device=DEV), cam_t, 64, 64)
    path = E.fit_angle(tensors, gids, hinge, target, cam_t, 64, 64, E.THETA_0, E.LR, E.STEPS, E.DECAY)
    assert len(path) == E.STEPS + 1 and 10 <= E.STEPS < 100
    print("\nrecovery: " + " ".join(f"{a:.4f}" for a in path), end="")
    assert abs(path[-1] - E.THETA_STAR) <= 0.25 * abs(E.THETA_0 - E.THETA_STAR)
