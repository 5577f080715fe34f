"""CPU: the scheduling policy of ``tts_batches`` (cosyvoice_amd/pipeline.py) — decode-job sizes and admission, the pipeline depth,
flow grouping, row splitting — driven the way the pipeline drives it, without a device or the library."""
import itertools
from collections import deque

import pytest
import torch

from cosyvoice_amd.pipeline import Admission, CuPartition, depth, flow_group, split_rows

RAMPS = ((2, 3, 3), (1, 2, 2, 3))


def _drive(n_batches, rows, max_batch, merge, ramp, n_llm):
    """The calling thread's loop: admit jobs while allowed, then retire one batch -> (job sizes, most batches drawn and not yet retired)."""
    adm = Admission(n_llm, merge, ramp, max_batch)
    it = iter([dict(texts=[None] * rows) for _ in range(n_batches)])
    held = {"now": 0, "peak": 0}

    def draw():
        b = next(it, None)
        if b is not None:
            held["now"] += 1
            held["peak"] = max(held["peak"], held["now"])
        return b
    nxt, inflight, sizes = draw(), 0, []
    while nxt is not None or inflight:
        while nxt is not None and adm.admits(inflight):
            bs, nxt = adm.fill(nxt, draw)
            inflight += len(bs)
            sizes.append(len(bs))
        inflight -= 1
        held["now"] -= 1
    assert held["now"] == 0 and sum(sizes) == n_batches
    return sizes, held["peak"]


@pytest.mark.parametrize("case,expected", [
    ((32, 8, 32, 4, (2, 3, 3), 2), [2, 3, 3, 4, 4, 4, 4, 4, 4]),
    ((10, 2, 4, 1, (1, 2, 2, 3), 2), [1] * 10),
    ((9, 2, 8, 3, (1, 2, 2, 3), 2), [1, 2, 2, 3, 1]),
    ((5, 2, 4, 3, (1, 2, 2, 3), 1), [1, 2, 2]),      # the row cap clips the job
])
def test_job_sizes_equal_the_inline_loop_they_replace(case, expected):
    assert _drive(*case)[0] == expected


def test_job_size_by_number():
    adm = Admission(2, 3, (1, 2, 2, 3, 9), 32)
    assert [adm.job_size(n) for n in range(7)] == [1, 2, 2, 3, 3, 3, 3]
    assert adm.admits(0) and adm.admits(11) and not adm.admits(12)   # the first job takes one batch: 11 + 1 <= (2 + 2) * 3


@pytest.mark.parametrize("n_llm,merge,ramp", list(itertools.product((1, 2, 3), (1, 2, 3, 4), RAMPS)))
def test_depth_is_reached_and_never_exceeded(n_llm, merge, ramp):
    from cosyvoice_amd.model import CosyVoice2Model
    d = depth(n_llm, merge)
    assert d == (n_llm + 2) * merge + 1
    _, peak = _drive(2 * d + 3, 1, 64, merge, ramp, n_llm)
    assert peak == d
    m = CosyVoice2Model.__new__(CosyVoice2Model)   # no stages, no weights: the method reads three plain attributes
    m.llm_cu_slots, m.llm_loops, m.llm_merge = 8, 2, merge
    assert m.tts_batches_depth(llm_loops=n_llm) == d and m.tts_batches_depth() == depth(2, merge)
    assert m.tts_batches_depth(llm_cu_slots=0) == depth(0, merge) == 2   # shared CUs: one batch decoding, one pending


def test_defaults_and_benchmark_settings():
    assert depth(2, 1) == 5 and depth(2, 4) == 17


def test_oversize_batch_is_refused():
    adm = Admission(2, 2, (), 4)
    with pytest.raises(ValueError, match="a batch of 5 utterances exceeds the LLM's max_batch 4"):
        adm.fill(dict(texts=[None] * 5), lambda: None)


class _Fut:
    def __init__(self, done=True, exc=None):
        self._done, self._exc = done, exc

    def done(self):
        return self._done

    def exception(self):
        return self._exc


def _entry(fut=None, n_p=10, ragged=False):
    B = 2
    b = dict(flow_prompt_speech_tokens=torch.zeros(B, n_p), prompt_speech_feats=torch.zeros(B, 2 * n_p, 80), flow_embeddings=torch.zeros(B, 192))
    if ragged:
        b["flow_prompt_speech_tokens"] = list(b["flow_prompt_speech_tokens"])
        b["prompt_speech_feats"] = list(b["prompt_speech_feats"])
    return dict(b=b, lf=fut or _Fut())


def _group(entries, fmerge):
    q = deque(entries)
    grp = flow_group(q.popleft(), q, fmerge)
    assert grp + list(q) == entries    # a prefix, in order; the rest stays queued
    return len(grp)


def test_flow_group_stops():
    assert _group([_entry() for _ in range(5)], 3) == 3                                       # flow_merge
    assert _group([_entry() for _ in range(2)], 3) == 2                                       # the queue ends
    assert _group([_entry(), _entry(), _entry(_Fut(done=False)), _entry()], 4) == 2           # tokens not there yet
    assert _group([_entry(), _entry(_Fut(exc=RuntimeError("decode"))), _entry()], 4) == 1     # a failed decode job
    assert _group([_entry(), _entry(), _entry(n_p=12), _entry(n_p=12)], 4) == 2               # another prompt length
    assert _group([_entry(), _entry(ragged=True), _entry()], 4) == 1                          # per-utterance prompt lists never merge
    assert _group([_entry(ragged=True), _entry(ragged=True)], 4) == 1
    # the oldest batch is the group's head whatever its future says: the flow thread waits for it
    assert _group([_entry(_Fut(done=False)), _entry(_Fut(done=False))], 4) == 1
    assert _group([_entry(_Fut(done=False)), _entry()], 4) == 2


def test_split_rows():
    wav, done = torch.arange(12.).view(6, 2), object()
    assert split_rows(wav, [6], done) == [(wav, done)] and split_rows(wav, [6], done)[0][0] is wav
    parts = split_rows(wav, [2, 1, 3], None)
    assert [p.shape[0] for p, _ in parts] == [2, 1, 3] and all(d is None for _, d in parts)
    assert torch.equal(torch.cat([p for p, _ in parts]), wav)
    rows = [torch.full((i + 1,), float(i)) for i in range(5)]
    assert split_rows(rows, [5], done) == [(rows, done)]
    assert split_rows(rows, [2, 3], done) == [(rows[:2], done), (rows[2:], done)]


def test_cu_partition_fields():
    assert CuPartition._fields == ("llm", "flow", "borrow", "prefill", "hift")
    llm, flow, borrow, prefill, hift = CuPartition([1, 2], 3, 4, [5, 6], 7)
    assert (llm, flow, borrow, prefill, hift) == ([1, 2], 3, 4, [5, 6], 7)
