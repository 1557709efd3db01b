"""splatfacto_groups: the five param groups of Trainer.KEYS carry splatfacto's default rates, its means schedule and the
features_dc / features_rest split of the one SH tensor (host-only: nothing is launched)."""
import pytest
import torch

from robosimgs_amd import GaussianAdam, Trainer, splatfacto_groups


def _params(n=7, k=16):
    return {"means": torch.zeros(n, 3), "quats": torch.zeros(n, 4), "scales": torch.zeros(n, 3),
            "opacities": torch.zeros(n), "colors": torch.zeros(n, k, 3)}


def test_splatfacto_groups_default_rates_and_splits():
    p = _params()
    groups = splatfacto_groups(p)
    assert [g["name"] for g in groups] == list(Trainer.KEYS)
    by = {g["name"]: g for g in groups}
    for k in Trainer.KEYS:
        assert len(by[k]["params"]) == 1 and by[k]["params"][0] is p[k]
    assert by["means"]["lr"] == 1.6e-4 and by["means"]["lr_final"] == 1.6e-6 and by["means"]["decay_steps"] == 30000
    assert by["quats"]["lr"] == 1e-3 and by["scales"]["lr"] == 5e-3 and by["opacities"]["lr"] == 5e-2
    assert by["colors"]["lr"] == 2.5e-3 and by["colors"]["head_floats"] == 3
    assert by["colors"]["rest_lr_scale"] == pytest.approx(1 / 20, rel=1e-15)
    for k in ("quats", "scales", "opacities", "colors"):
        assert "decay_steps" not in by[k] and "lr_final" not in by[k]            # constant: the optimiser's defaults
    # as GaussianAdam sees them: every per-group option is filled in, nothing but means decays or splits
    opt = GaussianAdam(groups, eps=1e-15, selective=True)
    got = {g["name"]: g for g in opt.param_groups}
    for k in Trainer.KEYS:
        assert set(("lr", "lr_final", "decay_steps", "head_floats", "rest_lr_scale")) <= set(got[k])
    assert [got[k]["decay_steps"] for k in Trainer.KEYS] == [30000, 0, 0, 0, 0]
    assert [got[k]["head_floats"] for k in Trainer.KEYS] == [0, 0, 0, 0, 3]
    assert opt.eps == 1e-15 and opt.betas == (0.9, 0.999) and opt.selective


def test_splatfacto_groups_overrides_and_a_degree_0_tensor():
    p = _params(k=1)
    by = {g["name"]: g for g in splatfacto_groups(p, means_lr=1e-3, means_lr_final=1e-5, decay_steps=100,
                                                  features_dc_lr=1e-2, features_rest_lr=1e-3, opacities_lr=0.1)}
    assert (by["means"]["lr"], by["means"]["lr_final"], by["means"]["decay_steps"]) == (1e-3, 1e-5, 100)
    assert by["opacities"]["lr"] == 0.1 and by["colors"]["lr"] == 1e-2
    assert by["colors"]["head_floats"] == 0 and by["colors"]["rest_lr_scale"] == 1.0      # [N, 1, 3]: features_dc only
    by = {g["name"]: g for g in splatfacto_groups(_params(k=9), features_dc_lr=1e-2, features_rest_lr=1e-3)}
    assert by["colors"]["head_floats"] == 3 and by["colors"]["rest_lr_scale"] == pytest.approx(0.1, rel=1e-15)


def test_state_dict_carries_the_counter_slot_before_the_first_step():
    opt = GaussianAdam(splatfacto_groups(_params()))
    sd = opt.state_dict()
    assert sd["step_state"] is None and sd["state"] == {} and len(sd["param_groups"]) == 5
    opt.load_state_dict(sd)
    assert opt.steps_taken() == 0
