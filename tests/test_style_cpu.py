"""CPU: the restatement of the 512-d speaker encoder (tests/style_ref.py) against the goldens minted from the reference's own
modules (tests/golden/style_*.npz), the key list against weights.speaker_embedding_specs(), and the teeth of the tolerances: each of
five injected faults moves the stage it acts on past that stage's tolerance on the committed cases."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_ref as R  # noqa: E402
from test_style_gpu import GOLDEN, TOL, load_case  # noqa: E402

CASES = ("style_t100", "style_t300", "style_wo_t100")


@pytest.fixture(scope="module")
def sds():
    from cosyvoice_amd.weights import speaker_embedding_state_dict
    return {True: speaker_embedding_state_dict(1986), False: speaker_embedding_state_dict(1986, post_enc=False)}


def _golden_errors(out, c):
    """Relative error of every stored stage against the golden, by the stage's own max |value| in the reference."""
    fx = c["fx"]
    err = {k: float(np.abs(out[k].double().numpy() - fx[k]).max() / np.abs(fx[k]).max()) for k in ("style_vec", "gst_out", "g")}
    if c["post"]:
        idx = torch.from_numpy(fx["row_idx"])
        err["m"] = float(np.abs(out["m"][idx].double().numpy() - fx["m_rows"]).max() / fx["m_absmax"])
        err["logs"] = float(np.abs(out["logs"][idx].double().numpy() - fx["logs_rows"]).max() / fx["logs_absmax"])
    return err


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference_goldens(sds, tag):
    c = load_case(tag)
    if c["post"]:                                    # the noise the reference was handed, regenerated from its seed
        nz = c["noise"].double()
        assert np.allclose([float(nz.sum()), float(nz.pow(2).sum()), float(nz[:, -1].sum())], c["fx"]["noise_checksum"], rtol=1e-12, atol=0)
    out = R.speaker_embedding(sds[c["post"]], c["wave"], c["n"], c["noise"], c["timbre"], post_enc=c["post"])
    assert out["spec"].shape == (c["n"] // 300, 513)
    for k, e in _golden_errors(out, c).items():
        assert e <= TOL[tag][k], (k, e, TOL[tag][k])


def test_bf16x3_products_stay_near_the_exact_ones(sds):
    c = load_case("style_t100")
    exact = R.speaker_embedding(sds[True], c["wave"], c["n"], c["noise"], c["timbre"], dtype=torch.float64)
    x3 = R.speaker_embedding(sds[True], c["wave"], c["n"], c["noise"], c["timbre"], products="bf16x3")
    for k in ("m", "style_vec"):                     # three bf16 products carry ~2^-16 per term
        e = float((x3[k].double() - exact[k]).abs().max() / exact[k].abs().max())
        assert 0 < e < 2e-4, (k, e)


def test_key_list_matches_specs():
    from cosyvoice_amd.weights import speaker_embedding_specs, speaker_embedding_state_dict  # noqa: F401
    fx = np.load(os.path.join(GOLDEN, "style_keys.npz"))
    ref = [(k, tuple(s)) for k, s in json.loads(str(fx["keys"]))]
    specs = speaker_embedding_specs()
    assert ref == [(k, tuple(s)) for k, s, _, _ in specs]
    n = sum(int(np.prod(s)) for k, s, kind, _ in specs if kind != "count" and "running_" not in k)
    total = sum(int(np.prod(s)) for k, s, kind, _ in specs if kind != "count")
    # 71.9 M trainable parameters as the reference module counts them; 72.0 M with the BatchNorm running statistics of CAM++
    assert n == int(fx["n_params"]) == 71910176 and round(total / 1e6, 1) == 72.0, (n, total)
    wo = [k for k, _, _, _ in speaker_embedding_specs(post_enc=False)]
    assert wo[:2] == ["enc_q.weight", "enc_q.bias"] and wo[2:] == [k for k, _ in ref if not k.startswith("enc_q.")]


def test_state_dict_order_and_removed_weight_norm(sds):
    from cosyvoice_amd.weights import campplus_state_dict, fold_weight_norm, speaker_embedding_specs
    sd = sds[True]
    assert list(sd) == [k for k, _, _, _ in speaker_embedding_specs()]
    cam = campplus_state_dict(1986)
    assert all(torch.equal(sd["speaker_encoder." + k], v) for k, v in cam.items())
    plain = {k: v for k, v in sd.items() if not k.endswith(("weight_g", "weight_v"))}
    for i in range(16):
        for n in (f"enc_q.enc.in_layers.{i}", f"enc_q.enc.res_skip_layers.{i}"):
            plain[n + ".weight"] = fold_weight_norm(sd, n)
    c = load_case("style_t100")
    a = R.speaker_embedding(sd, c["wave"], c["n"], c["noise"], c["timbre"])
    b = R.speaker_embedding(plain, c["wave"], c["n"], c["noise"], c["timbre"])
    assert float((a["g"] - b["g"]).abs().max()) <= TOL["style_t100"]["g"] * float(a["g"].abs().max())


# fault -> the stage it acts on (the first stored stage downstream of it) and the cases that have that stage
TEETH = [("mask+1", "m", "style_t100"), ("tap", "m", "style_t100"), ("gate_swap", "m", "style_t100"), ("mha_scale", "style_vec", "style_t100"),
         ("gst_tokens", "gst_out", "style_t100"), ("mask+1", "style_vec", "style_wo_t100"), ("tap", "style_vec", "style_wo_t100"),
         ("mha_scale", "style_vec", "style_wo_t100"), ("gst_tokens", "gst_out", "style_wo_t100")]


@pytest.mark.parametrize("fault,stage,tag", TEETH)
def test_injected_fault_exceeds_the_tolerance_of_its_stage(sds, fault, stage, tag):
    c = load_case(tag)
    out = R.speaker_embedding(sds[c["post"]], c["wave"], c["n"], c["noise"], c["timbre"], post_enc=c["post"], fault=fault)
    T = c["n"] // 300
    for k in ("m", "logs"):
        if k in out:
            out[k] = out[k][:T]
    e = _golden_errors(out, c)[stage]
    assert e > TOL[tag][stage], (fault, stage, e, TOL[tag][stage])
    print(f"{fault} on {tag}: {stage} moves by {e:.2e}, tolerance {TOL[tag][stage]:.2e}")
