"""Scenes, fp64 references and gates shared by tests/test_gpu_feature_channels.py, tests/test_gpu_operators_multi_camera.py
and tests/test_feature_channels_host.py (a helper module, not a test file).

The blend is linear and independent per feature channel: column c of the fp64 oracle's frame for features [N, 32] IS the
oracle's column c for any channel count that includes it, and alpha, last_ids, the margins and the flip weights do not
depend on the features at all.  So one run of O.rasterize per camera (32 channels, no background) serves every channel
count: `BlendReference.frame(ch, bg)` takes the first `ch` columns and adds T * bg with T = 1 - alpha.
tests/test_feature_channels_host.py checks that shortcut against the literal call O.rasterize(colors[N, ch], background=bg).
"""
import dataclasses
import math

import numpy as np

from oracle import gs_oracle_np as O

# every with_channels instantiation (csrc/mgs_common.h: 1, 2, 3, 4, 8, 16, 32); each wide bucket at its first count,
# an interior / last one and its exact size
CHANNELS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
MAX_CH = 32
TILE = 16
# one frame that is a whole number of tiles, one ragged in both axes (partial tiles on the right and the bottom edge)
FRAMES = {"tiles": dict(n=4000, mu=0.1, w=112, h=80, theta=0.3, seed=0),
          "ragged": dict(n=3000, mu=0.12, w=97, h=83, theta=0.3, seed=0)}
# the multi-camera operators: three ring cameras, frame ragged in both axes
MULTI = dict(n=3000, mu=0.12, w=97, h=83, seed=0, n_cams=3)
MULTI_SETUPS = ("ring", "blind_middle", "empty_tail")
MULTI_CHANNELS = (3, 7)
LAST_IDS_AGREE = 0.999          # the share of pixels test_rasterize_matches_oracle asks for


def tiles_of(w, h):
    return -(-w // TILE), -(-h // TILE)


def features(n, seed=11):
    """Features [n, 32] and background [32] in [0, 1), float32; a channel count `ch` takes the first `ch` columns."""
    rng = np.random.default_rng(seed)
    return rng.random((n, MAX_CH)).astype(np.float32), rng.random(MAX_CH).astype(np.float32)


def cotangents(w, h, seed=12):
    """v_render [h, w, 32] and v_alphas [h, w] ~ N(0, 1), float32."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(h, w, MAX_CH)).astype(np.float32), rng.normal(size=(h, w)).astype(np.float32)


def multi_cameras(setup):
    """Three camera_ring cameras at MULTI's frame size.  "blind_middle": camera 1 looks away from the scene (no visible
    Gaussian, no key: the fill loop of offset_encode_kernel between two cameras' keys spans a whole camera);
    "empty_tail": camera 2's principal point is moved up and left, so its right and bottom tiles -- the last tiles of the
    last camera -- are empty (the fill loop after the last key)."""
    from robosimgs_amd import Camera, camera_ring
    w, h = MULTI["w"], MULTI["h"]
    cams = camera_ring(MULTI["n_cams"], w, h)
    if setup == "blind_middle":
        pos = cams[1].position
        cams[1] = Camera.look_at(pos, 2.0 * pos, (0.0, 0.0, 1.0), w, h, 60.0)
    elif setup == "empty_tail":
        cams[2] = dataclasses.replace(cams[2], cx=cams[2].cx - 0.6 * w, cy=cams[2].cy - 0.6 * h)
    elif setup != "ring":
        raise ValueError(setup)
    return cams


def scene(spec):
    from robosimgs_amd import synthetic_scene
    return synthetic_scene(spec["n"], math.log(spec["mu"]), 0, spec["seed"])


# ----------------------------------------------------------------------------------------------------------------------
# forward gate
# ----------------------------------------------------------------------------------------------------------------------
class BlendReference:
    """fp64 blend of ONE camera's lists on the given (fp32) inputs, with margins and flip weights under O.EPS_STAGE."""

    def __init__(self, means2d, conics, feats, opacities, flatten_ids, offsets, w, h):
        self.w, self.h = w, h
        self.feats = np.asarray(feats, np.float64)
        assert self.feats.shape[1] == MAX_CH
        self.offsets = np.asarray(offsets).reshape(tiles_of(w, h)[::-1])
        self.flatten_ids = np.asarray(flatten_ids)
        self.img, self.alpha, self.last, stats = O.rasterize(
            means2d, conics, self.feats, opacities, self.flatten_ids, self.offsets, w, h, TILE, background=None,
            margins=True, flip_eps=O.EPS_STAGE)
        self.margins, self.flip_weight, self.contribs = stats["margins"], stats["flip_weight"], stats["contribs"]
        ends = np.concatenate([self.offsets.reshape(-1)[1:], [len(self.flatten_ids)]])
        self.longest_list = int((ends - self.offsets.reshape(-1)).max())

    def frame(self, ch, bg=None, expected_last=False):
        """The oracle's frame [h, w, ch]: background at weight T = 1 - alpha; expected_last: the last channel divided by
        max(alpha, 1e-10) (A.2 step 9, as O.render does for the "ED" modes)."""
        img = self.img[..., :ch].copy()
        if bg is not None:
            img += (1.0 - self.alpha)[..., None] * np.asarray(bg, np.float64)[:ch]
        if expected_last:
            img[..., -1] /= np.maximum(self.alpha, 1e-10)
        return img

    def feat_max(self, ch, bg=None):
        fm = np.abs(self.feats[:, :ch]).max(axis=0)
        return fm if bg is None else np.maximum(fm, np.abs(np.asarray(bg, np.float64)[:ch]))


def check_forward(ref, ch, render, alphas, last_ids=None, bg=None, expected_last=False, what="frame"):
    """THE forward gate of these files: O.check_frame at tolerance 1e-4 under O.EPS_STAGE with the flip bound required
    (zero unexplained pixels, could-flip share under check_frame's 5 % cap), and last_ids equal to the oracle's on
    LAST_IDS_AGREE of the pixels.  Prints and returns check_frame's statistics."""
    render = np.asarray(render)
    assert render.shape == (ref.h, ref.w, ch), (render.shape, ch)
    st = O.check_frame(render, np.asarray(alphas), ref.frame(ch, bg, expected_last), ref.alpha, ref.margins, O.EPS_STAGE,
                       expected_depth=expected_last, what=what, flip_weight=ref.flip_weight, feat_max=ref.feat_max(ch, bg),
                       require_flip_bound=True)
    if last_ids is not None:
        same = float((np.asarray(last_ids) == ref.last).mean())
        st["last_ids_agree"] = same
        assert same >= LAST_IDS_AGREE, f"{what}: last_ids agree on {same:.5f} of pixels"
    print(f"\n{what}: could-flip {st['could_flip_frac']:.2e}, over 1e-4 {st['over_tol']} (unexplained {st['unexplained']}), "
          f"max err off flips {st['max_err_nonflip']:.2e}, flip over bound {st['flip_over_bound']}"
          + (f", last_ids agree {st['last_ids_agree']:.5f}" if last_ids is not None else ""))
    return st


# ----------------------------------------------------------------------------------------------------------------------
# backward reference: fp64 autograd through the torch oracle
# ----------------------------------------------------------------------------------------------------------------------
class BackwardReference:
    """fp64 autograd through OT.rasterize on the given lists.  The graph is built once at 32 channels without a background;
    a channel count takes the first `ch` columns of the frame (and of v_feats), a background enters as T * bg with
    T = 1 - alpha, the expected last channel as img[..., -1] / clamp(alpha, 1e-10)."""

    def __init__(self, means2d, conics, feats, opacities, flatten_ids, offsets, w, h, dtype=None):
        import torch
        from oracle import gs_oracle_torch as OT
        dtype = dtype or torch.float64
        leaf = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
        self.dtype = dtype
        self.leaves = [leaf(means2d), leaf(conics), leaf(feats), leaf(opacities)]
        offs = np.asarray(offsets).reshape(tiles_of(w, h)[::-1])
        self.img, self.alpha = OT.rasterize(*self.leaves, np.asarray(flatten_ids), offs, w, h, TILE, None)

    def grads(self, ch, v_render, v_alphas, bg=None, expected_last=False):
        """(v_means2d [N,2], v_conics [N,3], v_feats [N,ch], v_opacities [N,1]) -- and v_background [1,ch] behind them when a
        background is given -- of <v_render, frame> + <v_alphas, alpha>, as float64 arrays."""
        import torch
        img = self.img[..., :ch]
        bg_leaf = None
        if bg is not None:
            bg_leaf = torch.tensor(np.asarray(bg)[:ch], dtype=self.dtype, requires_grad=True)
            img = img + (1.0 - self.alpha)[..., None] * bg_leaf
        if expected_last:
            img = torch.cat([img[..., :-1], (img[..., -1] / torch.clamp(self.alpha, min=1e-10))[..., None]], dim=-1)
        loss = (img * torch.tensor(np.asarray(v_render)[..., :ch], dtype=self.dtype)).sum()
        if v_alphas is not None:
            loss = loss + (self.alpha * torch.tensor(np.asarray(v_alphas), dtype=self.dtype)).sum()
        g = torch.autograd.grad(loss, self.leaves + ([bg_leaf] if bg is not None else []), retain_graph=True)
        g = [x.double().numpy() for x in g]
        return (g[0], g[1], g[2][:, :ch], g[3].reshape(-1, 1)) + ((g[4].reshape(1, -1),) if bg is not None else ())


# ----------------------------------------------------------------------------------------------------------------------
# multi-camera lists
# ----------------------------------------------------------------------------------------------------------------------
def multi_camera_lists(means2d, radii, depths, tw, th):
    """What ops.isect_tiles / ops.isect_offset_encode must return for [C, N, ...] inputs: the concatenation over c of
    O.isect_tiles(..., cam=c, n_cams=C, dtype=np.float32) with + c * N on the ids, and O.isect_offsets of the keys.
    Returns (tiles_per_gauss [C,N], keys int64, flatten_ids int32, offsets [C,th,tw])."""
    C, N = np.asarray(depths).shape
    tpg, keys, ids = [], [], []
    for c in range(C):
        t, k, f = O.isect_tiles(means2d[c], radii[c], depths[c], TILE, tw, th, cam=c, n_cams=C, dtype=np.float32)
        tpg.append(t)
        keys.append(k)
        ids.append(f.astype(np.int64) + c * N)
    keys = np.concatenate(keys)
    return np.stack(tpg), keys, np.concatenate(ids).astype(np.int32), O.isect_offsets(keys, C, tw, th)


def check_lists(got, ref, what="lists"):
    """got / ref: (tiles_per_gauss, keys, flatten_ids, offsets).  Element for element; keys ascending over the whole array."""
    names = ("tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets")
    for name, g_, r_ in zip(names, got, ref):
        g_, r_ = np.asarray(g_), np.asarray(r_)
        assert g_.shape == r_.shape, f"{what}: {name} shape {g_.shape} != {r_.shape}"
        np.testing.assert_array_equal(g_, r_, err_msg=f"{what}: {name}")
    keys = np.asarray(got[1])
    assert np.all(keys[1:] >= keys[:-1]), f"{what}: keys are not ascending"
    C = np.asarray(got[3]).shape[0]
    off = np.concatenate([np.asarray(got[3]).reshape(-1), [len(keys)]])
    assert off[0] == 0 and np.all(np.diff(off) >= 0), f"{what}: offsets are not monotone"
    return dict(n_isect=int(len(keys)), per_camera=[int(off[(c + 1) * (len(off) - 1) // C] - off[c * (len(off) - 1) // C])
                                                    for c in range(C)])


def camera_lists(flatten_ids, offsets, c, n):
    """Camera c's own lists out of the concatenated ones: (ids local to the camera [n_c], offsets [th,tw] from 0)."""
    offsets = np.asarray(offsets)
    C = offsets.shape[0]
    flat = np.concatenate([offsets.reshape(-1), [len(flatten_ids)]]).astype(np.int64)
    n_tiles = offsets[0].size
    s, e = flat[c * n_tiles], flat[(c + 1) * n_tiles]
    ids = np.asarray(flatten_ids[s:e]).astype(np.int64) - c * n
    assert C > c and (len(ids) == 0 or (ids.min() >= 0 and ids.max() < n)), f"camera {c}: ids outside its own rows"
    return ids.astype(np.int32), (offsets[c].astype(np.int64) - s).astype(np.int32)
