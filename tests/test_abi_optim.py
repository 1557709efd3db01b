"""The optimiser's boundary: include/mgs_optim.h <-> libmgs.so / libmgs_debug.so <-> the second ctypes table
(_lib.OPTIM_EXPORTS), and mgs_adam_step's argument checks (no compute calls here: CPU-only)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_optim.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_optim_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.OPTIM_EXPORTS) == ["mgs_adam_step"]
    assert not set(_lib.OPTIM_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 29
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+MGS_ADAM_MAX_GROUPS\s+(\d+)", header).group(1)) == _lib.ADAM_MAX_GROUPS == 8
    assert "MGS_VERSION" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)      # the version is mgs.h's alone


def test_adam_group_struct_matches_the_header():
    """The ctypes structure has the header's fields, in its order, at a C compiler's offsets."""
    from robosimgs_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct mgs_adam_group \{(.*?)\} mgs_adam_group;", src, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.AdamGroup._fields_]
    G = _lib.AdamGroup
    assert [getattr(G, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44, 48, 56, 64, 72] and ctypes.sizeof(G) == 80


def _group(**kw):
    from robosimgs_amd import _lib
    f = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000, n=10, row_floats=3, head_floats=0, lr=1e-3,
             lr_final=1e-3, decay_steps=0, rest_lr_scale=1.0)
    f.update(kw)
    return _lib.AdamGroup(**f)


def _call(groups, n_groups=None, beta1=0.9, beta2=0.999, eps=1e-8, state=0x5000, radii=None, radii_y=None, n_cams=0,
          cam_stride=0, mask=None):
    """mgs_adam_step on made-up addresses: every case here must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    table = (_lib.AdamGroup * len(groups))(*groups)
    rc = L.mgs_adam_step(len(groups) if n_groups is None else n_groups, table, beta1, beta2, eps, state, radii, radii_y,
                         n_cams, cam_stride, mask, None)
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(groups=[_group] * 9), b"n_groups"),
    (dict(groups=[_group], n_groups=0), b"n_groups"),
    (dict(groups=[lambda: _group(row_floats=0)]), b"row_floats"),
    (dict(groups=[lambda: _group(head_floats=4)]), b"head_floats"),
    (dict(groups=[_group], beta1=1.0), b"beta1"),
    (dict(groups=[_group], beta1=-0.1), b"beta1"),
    (dict(groups=[_group], beta2=1.0), b"beta2"),
    (dict(groups=[lambda: _group(param=0x1004)]), b"param"),
    (dict(groups=[lambda: _group(grad=0x2008)]), b"grad"),
    (dict(groups=[lambda: _group(exp_avg=0x3001)]), b"exp_avg "),
    (dict(groups=[_group, lambda: _group(exp_avg_sq=0x400c)]), b"groups[1].exp_avg_sq"),
    (dict(groups=[_group], radii=0x6000, n_cams=1, cam_stride=10, mask=0x7000), b"radii and mask"),
])
def test_adam_step_argument_errors_are_reported_without_a_gpu(kw, word):
    kw = dict(kw, groups=[g() for g in kw["groups"]])
    rc, msg = _call(**kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_further_argument_errors():
    """What else cannot be launched: a second radii axis without the first, radii without cameras, groups of different
    row counts under a mask, a schedule towards a non-positive rate, no counter."""
    for kw, word in ((dict(groups=[_group()], radii_y=0x6000), b"radii_y"),
                     (dict(groups=[_group()], radii=0x6000, n_cams=0), b"n_cams"),
                     (dict(groups=[_group(), _group(n=11)], mask=0x7000), b"groups[1].n"),
                     (dict(groups=[_group()], radii=0x6000, n_cams=2, cam_stride=9), b"cam_stride"),
                     (dict(groups=[_group(decay_steps=5, lr_final=0.0)]), b"lr_final"),
                     (dict(groups=[_group(n=1 << 31, row_floats=2)]), b"row_floats"),
                     (dict(groups=[_group()], state=None), b"step_state")):
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_gaussian_adam_is_exported_lazily_and_refuses_cpu_tensors():
    import torch
    import robosimgs_amd
    from robosimgs_amd import GaussianAdam, splatfacto_groups
    from robosimgs_amd._lib import MgsError
    assert GaussianAdam is robosimgs_amd.optim.GaussianAdam and callable(splatfacto_groups)
    assert issubclass(GaussianAdam, torch.optim.Optimizer)
    p = torch.zeros(5, 3, requires_grad=True)
    opt = GaussianAdam([p], lr=1e-2)
    opt.step()                                   # no gradient anywhere: nothing to launch
    p.grad = torch.ones_like(p)
    with pytest.raises(MgsError, match="CPU tensor"):
        opt.step()
    with pytest.raises(MgsError, match="visibility"):
        GaussianAdam([p], selective=True).step()
    with pytest.raises(ValueError, match="betas"):
        GaussianAdam([p], betas=(0.9, 1.0))
