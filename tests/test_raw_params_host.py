"""The raw parameter form (include/mgs.h MGS_PARAMS_RAW: `scales` are log-scales, `opacities` logits) as far as it is
reachable without a GPU: the flag constants, the argument errors, the training-state layout, the loaders and the
refusals of the Python layer.  What runs on the device is in tests/test_gpu_raw_params.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs.h")


def _defines():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MGS_(\w+)\s+(\d+)\b", open(HEADER).read(), flags=re.M)}


def test_the_flag_is_one_free_bit_of_both_flags_words():
    from robosimgs_amd import ops
    d = _defines()
    raw = d["PARAMS_RAW"]
    assert raw == ops.PARAMS_RAW == 64 and raw & (raw - 1) == 0
    assert d["PARAMS_OPAC_PLAIN"] == ops.PARAMS_OPAC_PLAIN
    bin_bits = [v for k, v in d.items() if k.startswith("BIN_")] + [d["PARAMS_OPAC_PLAIN"]]
    frame_bits = [v for k, v in d.items() if k.startswith("FRAMES_")] + [d["RASTER_EXPECTED_LAST"], d["RASTER_LATENCY"]]
    for word in (bin_bits, frame_bits):
        assert all(raw & v == 0 for v in word), word
        assert len(set(word)) == len(word) and all(v & (v - 1) == 0 for v in word)      # one bit each, none shared
    assert all(raw & v == 0 for k, v in d.items() if k.startswith("CAMERA_"))    # mgs_project_color_bwd's camera_model word


def test_frames_flags_sets_that_bit_and_nothing_else():
    from robosimgs_amd import ops
    for args in ((False, False, True, False, 0), (True, True, False, True, 2), (True, False, True, False, 1)):
        assert ops.frames_flags(*args, raw=True) == ops.frames_flags(*args) | ops.PARAMS_RAW
        assert ops.frames_flags(*args, raw=False) == ops.frames_flags(*args)
        assert ops.frames_flags(*args) & ops.PARAMS_RAW == 0
    assert ops.frames_flags(False, False, True, False, 0, raw=True) == ops.PARAMS_RAW
    for fn in (ops.project_color_fwd_raw, ops.project_color_bwd_raw, ops.render_frames_raw, ops.render_frames_train_raw,
               ops.render_frames_backward_raw, ops.frames_flags, ops.TrainState.__init__):
        par = list(inspect.signature(fn).parameters.values())
        assert par[-1].name == "raw" and par[-1].default is False, fn          # trailing, default = today's behaviour


def test_raw_without_logits_is_an_argument_error_not_a_fault():
    """MGS_PARAMS_RAW with NULL opacities: MGS_ERR_INVALID_ARGUMENT naming the flag, before any launch (every pointer
    here is NULL, so a launch would be a fault)."""
    from robosimgs_amd import _lib, ops
    L = _lib.lib()
    raw = ops.PARAMS_RAW
    rc = L.mgs_project_color_fwd(4, None, None, None, None, 0, 1, None, None, None, 16, 16, 0.3, 0.01, 1e10, 0.0, None, None, None,
                                 None, None, 3, None, None, raw, None, None, None, None)
    assert rc == -1 and b"MGS_PARAMS_RAW" in L.mgs_last_error_string()
    nbytes = ctypes.c_size_t(0)
    rc = L.mgs_render_frames(4, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, 0.3, 0.01, 1e10, 0.0, 0, 3, raw, None,
                             100, None, None, None, None, None, None, 0, None, None, ctypes.byref(nbytes), None)
    assert rc == -1 and b"MGS_PARAMS_RAW" in L.mgs_last_error_string()
    rc = L.mgs_render_frames_train(4, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, 0.3, 0.01, 1e10, 0.0, 0, 3, raw,
                                   None, 100, 0, None, None, None, None, ctypes.byref(nbytes), None)
    assert rc == -1 and b"MGS_PARAMS_RAW" in L.mgs_last_error_string()
    rc = L.mgs_render_frames_backward(4, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, 0.3, 0, 3, raw, None, 100, 0,
                                      None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                      ctypes.byref(nbytes), None)
    assert rc == -1 and b"MGS_PARAMS_RAW" in L.mgs_last_error_string()
    # mgs_project_color_bwd takes the forward's bit in its camera_model word (MGS_CAMERA_* | MGS_PARAMS_RAW)
    args = [4] + [None] * 4 + [0, 1, None, None, None, 16, 16, 0.3, None, None, 0, 3] + [None] * 12 + [0]
    assert len(args) + 2 == len(L.mgs_project_color_bwd.argtypes)
    rc = L.mgs_project_color_bwd(*args, ops.CAMERA_MODELS["fisheye"] | raw, None)
    assert rc == -1 and b"MGS_PARAMS_RAW" in L.mgs_last_error_string()
    rc = L.mgs_project_color_bwd(*args, 3 | raw, None)                         # 3 is no camera model, with or without the bit
    assert rc == -1 and b"camera_model" in L.mgs_last_error_string()
    # without the bit the same calls fail on something else (the checks above are the flag's)
    rc = L.mgs_project_color_fwd(4, None, None, None, None, 0, 1, None, None, None, 16, 16, 0.3, 0.01, 1e10, 0.0, None, None, None,
                                 None, None, 3, None, None, 0, None, None, None, None)
    assert rc == -1 and b"MGS_PARAMS_RAW" not in L.mgs_last_error_string()


def test_train_state_keeps_the_opacity_field_in_raw_form():
    """mgs_train_state_layout(antialiased=...) means "the opacity field is kept": ops.TrainState asks for it in raw form
    whether anti-aliased or not, and for nothing else to move."""
    from robosimgs_amd import _lib, ops
    L = _lib.lib()
    n, W, H, ch, cap, S = 100_000, 640, 368, 4, 500_000, 64
    lay = {}
    for keep in (0, 1):
        offs = (ctypes.c_size_t * len(ops.TRAIN_FIELDS))()
        per = ctypes.c_size_t(0)
        assert L.mgs_train_state_layout(n, W, H, ch, cap, keep, S, offs, ctypes.byref(per)) == 0
        lay[keep] = (dict(zip(ops.TRAIN_FIELDS, offs)), per.value)
    size = lambda o, per, f: (o[ops.TRAIN_FIELDS[ops.TRAIN_FIELDS.index(f) + 1]] - o[f])
    assert size(*lay[1], "opac_aa") >= 4 * n > size(*lay[0], "opac_aa")
    assert len(ops.TRAIN_FIELDS) == 17 and lay[1][1] - lay[0][1] == size(*lay[1], "opac_aa") - size(*lay[0], "opac_aa")
    dev = torch.device("cpu")                                                  # (the layout is host arithmetic)
    flags = ops.frames_flags(True, True, True, False, 0, raw=True)
    plain = ops.TrainState(n, 1, W, H, ch, cap, False, S, flags & ~ops.PARAMS_RAW, dev)
    raw = ops.TrainState(n, 1, W, H, ch, cap, False, S, flags, dev, raw=True)
    raw_aa = ops.TrainState(n, 1, W, H, ch, cap, True, S, flags, dev, raw=True)
    assert plain.offsets == list(lay[0][0].values()) and raw.offsets == raw_aa.offsets == list(lay[1][0].values())
    assert raw.views(0)["opac_aa"].shape == (n,) and plain.views(0)["opac_aa"].shape == (0,)
    assert raw.antialiased is False and raw.raw and not plain.raw


def test_to_torch_raw_hands_out_the_stored_arrays(tmp_path):
    from robosimgs_amd import synthetic_scene
    from robosimgs_amd.gaussians import load_ply, save_ply
    g = synthetic_scene(500, np.log(0.05), 2, 3)
    t = g.to_torch("cpu", raw=True)
    assert t["scales"].dtype == t["opacities"].dtype == torch.float32
    assert np.array_equal(t["scales"].numpy().view(np.uint32), np.asarray(g.log_scales, np.float32).view(np.uint32))
    assert np.array_equal(t["opacities"].numpy().view(np.uint32), np.asarray(g.opacity_logits, np.float32).view(np.uint32))
    a = g.to_torch("cpu")                                                      # the default is today's: activated
    assert np.array_equal(a["scales"].numpy(), g.scales) and np.array_equal(a["opacities"].numpy(), g.opacities)
    for k in ("means", "quats", "colors"):
        assert torch.equal(a[k], t[k])
    assert inspect.signature(g.to_torch).parameters["raw"].default is False
    path = str(tmp_path / "scene.ply")
    save_ply(path, g)
    t2 = load_ply(path).to_torch("cpu", raw=True)
    for k in ("means", "quats", "scales", "opacities", "colors"):
        assert torch.equal(t2[k], t[k]), k


def test_refusals_of_the_python_layer():
    from robosimgs_amd import FrameRenderer, Trainer, rasterization
    z = torch.zeros
    with pytest.raises(NotImplementedError, match="raw_params"):
        rasterization(z(4, 3), z(4, 4), z(4, 3), z(4), z(4, 3), z(1, 4, 4), z(1, 3, 3), 16, 16, sh_degree=None, raw_params=True)
    t = dict(means=z(4, 3), quats=z(4, 4), scales=z(4, 3), opacities=z(4), colors=z(4, 1, 3), sh_degree=0)
    with pytest.raises(ValueError, match="raw_params"):
        FrameRenderer(t, 16, 16, isect_capacity=100, group_ids=torch.zeros(4, dtype=torch.int32), n_groups=1, raw_params=True)
    assert inspect.signature(rasterization).parameters["raw_params"].default is False
    # Trainer forwards the keyword to its render call and keeps its keys
    seen = {}

    def fake(*a, **kw):
        seen.update(kw)
        return None, None, {}
    p = {k: z(4, 3) for k in Trainer.KEYS}
    Trainer(p, None, 16, 16, auto_reorder_every=0, render_fn=fake, raw_params=True, sh_degree=0).render(None, None)
    assert seen == {"raw_params": True, "sh_degree": 0}
    seen.clear()
    Trainer(p, None, 16, 16, auto_reorder_every=0, render_fn=fake, sh_degree=0).render(None, None)
    assert seen == {"sh_degree": 0}
    assert Trainer.KEYS == ("means", "quats", "scales", "opacities", "colors") and "raw_params" in Trainer.__doc__
