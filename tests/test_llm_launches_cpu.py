"""CPU: the launch sequences of ``Qwen2LM`` (cosyvoice_amd/llm.py) — every prefill / decode-step / request form — equal the recorded
ones exactly: order, op, every tensor argument (owner, storage offset, shape, strides, dtype) and every scalar.  The captured decode
graph is built from these Python sequences, so "same launches with the same arguments" is "same results and same graph": a
restructuring of llm.py that keeps this test green did not move behaviour.  No device and no library: ``llm.ops`` is a recorder.

A change that alters a sequence ON PURPOSE (a fused launch, another slab count) regenerates the stored traces with

    python -m tests.test_llm_launches_cpu        (from the repository root)

and commits the new tests/golden/llm_launches.json; its diff (one launch per line) is then the reviewable statement of what moved.
"""
import ctypes
import json
import os

import pytest
import torch

import cosyvoice_amd.llm as llm_mod
from cosyvoice_amd import ops as real_ops
from cosyvoice_amd.config import LlmConfig
from cosyvoice_amd.lora import LoraBank
from cosyvoice_amd.weights import llm_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llm_launches.json")
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.int32: "i32", torch.int64: "i64"}


class _Recorder:
    """Stands in for ``cosyvoice_amd.ops`` inside llm.py: constants pass through, every launch is appended to ``trace``."""

    def __init__(self, lm):
        self.lm, self.trace = lm, []

    def pack_skinny(self, W, interleave=False):
        return W.clone()

    def drop_graphs(self, *caches):
        pass

    def bound_cache(self, cache, key, *dependents, cap=None):
        pass

    def __getattr__(self, name):
        real = getattr(real_ops, name)
        if not callable(real):
            return real
        return lambda *a, **k: self.trace.append([name, [self._enc(v) for v in a], {n: self._enc(v) for n, v in k.items()}])

    def _owners(self):
        """storage pointer -> (name, bytes) of every long-lived tensor of the LM, its bank and its workspaces (first name wins)."""
        lm, out = self.lm, {}

        def add(name, t):
            if torch.is_tensor(t):
                out.setdefault(t.untyped_storage().data_ptr(), (name, t.untyped_storage().nbytes()))
        for k, t in lm.st.items():
            add(f"st.{k}", t)
        for i, lay in enumerate(lm.layers):
            for k, t in lay.items():
                add(f"layer{i}.{k}", t)
        for k in ("g_final", "embed_tokens", "llm_embedding", "speech_embedding", "dec_b", "p_dec", "inv_freq", "rope_table", "_k_rm", "_vt_rm"):
            add(k, getattr(lm, k))
        for i in range(len(lm.layers)):
            add(f"kcache{i}", lm.kcache[i])
            add(f"vtcache{i}", lm.vtcache[i])
        for key, ws in lm._prefill_ws.items():
            for k, t in ws.items():
                add(f"ws{list(key)}.{k}", t)
        if lm._lora is not None:
            bank = lm._lora["bank"]
            for k, t in lm._lora.items():
                add(f"lora.{k}", t)
            for key, ws in lm._lora["ws"].items():
                for k, t in ws.items():
                    add(f"lora_ws{list(key)}.{k}", t)
            for i, lay in enumerate(bank.layers):
                for k, t in lay.items():
                    add(f"bank.layer{i}.{k}", t)
            for k, t in vars(bank).items():
                add(f"bank.{k}", t)
        return out

    def _ptr(self, p):
        if not p:
            return None
        for base, (name, nbytes) in self._owners().items():
            if base <= p < base + nbytes:
                return f"{name}+{p - base}B"
        return "?"

    def _enc(self, v):
        if torch.is_tensor(v):
            name = self._owners().get(v.untyped_storage().data_ptr(), ("tmp", 0))[0]
            s = f"{name}@{v.storage_offset()}:{list(v.shape)}:{list(v.stride())}:{_DT[v.dtype]}"
            if name == "tmp" and not v.is_floating_point():
                s += f"={v.tolist()}"      # a small host-made index / length tensor (the ragged klen): its values are the argument
            return s
        if isinstance(v, ctypes.Structure):
            return {f: (self._ptr(getattr(v, f)) if t is ctypes.c_void_p else getattr(v, f)) for f, t in v._fields_}
        if isinstance(v, dict):
            return {k: self._enc(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self._enc(x) for x in v]
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        return v


def _lm(monkeypatch):
    torch.manual_seed(0)
    cfg = LlmConfig.tiny()
    lm = llm_mod.Qwen2LM(cfg, torch.bfloat16, "cpu", max_batch=32, ctx_max=128, max_out=64)
    rec = _Recorder(lm)
    monkeypatch.setattr(llm_mod, "ops", rec)
    lm.load_state_dict(llm_state_dict(cfg))
    lm.attach_lora(LoraBank(lm, 2, r=16))
    lm.use_graph = False
    return lm, rec


def _request():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    texts = [i32(5, 6, 7, 8, 9), i32(10, 11, 12)]
    prompt_texts = [i32(1, 2, 3), i32(4, 5)]
    prompt_speech = [i32(20, 21, 22, 23), i32(30, 31, 32)]
    return texts, prompt_texts, prompt_speech


def _with(lm, fn, **attrs):
    old = {k: getattr(lm, k) for k in attrs}
    for k, v in attrs.items():
        setattr(lm, k, v)
    try:
        fn()
    finally:
        for k, v in old.items():
            setattr(lm, k, v)


# form -> (launches of the tiny 2-layer configuration, how to run it)
FORMS = {
    "decode_B4": (13, lambda lm: lm._decode_step(4)),
    "decode_B12": (15, lambda lm: lm._decode_step(12)),
    "decode_B20": (15, lambda lm: lm._decode_step(20)),
    "decode_B4_no_split_norm": (13, lambda lm: _with(lm, lambda: lm._decode_step(4), split_norm=False)),
    "decode_B4_cu_budget64": (13, lambda lm: _with(lm, lambda: lm._decode_step(4), cu_budget=64)),
    "lora_decode_B4": (35, lambda lm: lm._decode_step(4, lora=True)),
    "lora_decode_B20": (35, lambda lm: lm._decode_step(20, lora=True)),
    "prefill_2x12": (21, lambda lm: lm._prefill(2, 12, False, False)),
    "prefill_2x12_ragged": (21, lambda lm: lm._prefill(2, 12, False, False, lens=[12, 9])),
    "lora_prefill_2x12": (39, lambda lm: lm._prefill(2, 12, False, False, lora=True)),
    "lora_prefill_2x12_ragged": (39, lambda lm: lm._prefill(2, 12, False, False, lens=[12, 9], lora=True)),
    "generate_batch": (50, lambda lm: lm.generate_batch(*_request(), max_steps=3)),
    "generate_batch_adapters": (114, lambda lm: lm.generate_batch(*_request(), max_steps=3, adapters=[0, -1])),
    "forced_logits_adapters": (114, lambda lm: lm.forced_logits(*[t[0] for t in _request()], [4, 5], rows=2, adapters=[1, -1])),
}


def _trace(lm, rec, form):
    rec.trace.clear()
    FORMS[form][1](lm)
    return json.loads(json.dumps(rec.trace))   # what a stored trace looks like after its round trip (tuples -> lists)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traced():
    mp = pytest.MonkeyPatch()
    try:
        yield _lm(mp)
    finally:
        mp.undo()


def test_golden_holds_exactly_the_forms(golden):
    assert sorted(golden) == sorted(FORMS)
    assert {k: len(v) for k, v in golden.items()} == {k: n for k, (n, _) in FORMS.items()}


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_sequence_equals_recorded(traced, golden, form):
    got, want = _trace(*traced, form), golden[form]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{form}: launch {i} differs"
    assert len(got) == len(want) == FORMS[form][0]


def test_every_tensor_argument_has_an_owner_or_is_a_host_made_index(golden):
    """The trace pins addresses only through owner names: nothing but the documented temporaries may be anonymous, no pointer unknown."""
    text = json.dumps(golden)
    assert '"?"' not in text
    anon = {s.split("=")[0] for s in _strings(golden) if s.startswith("tmp@")}
    # the ragged klen (2 sequences) and the gathered A^T rows of the embedding adapters (n tokens, r = 16)
    assert all(a.endswith(":i32") and a.startswith("tmp@0:[2]") or a.endswith(":[16, 1]:f32") for a in anon), anon


def _strings(v):
    if isinstance(v, str):
        yield v
    elif isinstance(v, dict):
        for x in v.values():
            yield from _strings(x)
    elif isinstance(v, list):
        for x in v:
            yield from _strings(x)


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    lm, rec = _lm(mp)
    out = {form: _trace(lm, rec, form) for form in FORMS}
    mp.undo()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(l, separators=(",", ":")) for l in v) + "\n]"
                                   for k, v in out.items()) + "\n}\n")
    print({k: len(v) for k, v in out.items()})
