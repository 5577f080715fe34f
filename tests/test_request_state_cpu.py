"""CPU: the per-request state that outlives a call — the pool of decode contexts of ``CosyVoice2Model`` across a reload, and the
streaming encoder caches of the flow under concurrent requests — with stand-in stages: no device, no library."""
import threading
from types import SimpleNamespace

import pytest
import torch

from cosyvoice_amd.config import FlowConfig
from cosyvoice_amd.flow import CausalMaskedDiffWithXvec
from cosyvoice_amd.model import CosyVoice2Model


# ------------------------------------------------------------------ decode contexts across a reload
@pytest.fixture
def model(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: object())
    m = CosyVoice2Model.__new__(CosyVoice2Model)   # no stages, no weights: the pool reads these attributes alone
    m.device, m.max_llm_requests = "cpu", 2
    m.llm = SimpleNamespace(new_context=lambda: SimpleNamespace(_graphs={}))
    m._req_pool_lock, m._req_pool, m._req_made, m._req_gen = threading.Condition(), [], 0, 0
    return m


def test_pair_taken_before_a_reload_is_discarded_on_release(model):
    m = model
    pair = m._acquire_llm()
    m._drop_contexts()                 # what load() / load_state_dicts() do first
    m._release_llm(pair)               # raises nothing
    assert m._req_pool == [] and m._req_made == 0
    fresh = m._acquire_llm()
    assert fresh[0] is not pair[0] and m._req_made == 1
    m._release_llm(fresh)
    assert m._req_pool == [fresh]


def test_stale_pair_does_not_join_the_pool_another_request_re_created(model):
    m = model
    old = m._acquire_llm()
    m._drop_contexts()
    new = m._acquire_llm()             # another request, after the reload
    m._release_llm(new)
    m._release_llm(old)
    assert m._req_pool == [new] and m._req_made == 1
    assert m._acquire_llm() is new     # later requests decode with the new weights' context
    assert m._acquire_llm()[0] is not old[0] and m._req_made == 2


def _blocked_acquire(m):
    """Start a thread that acquires a pair and wait until it sleeps at the cap -> (thread, its result list)."""
    asleep, got = threading.Event(), []
    wait = m._req_pool_lock.wait

    def waiting(*a):
        asleep.set()                   # still holds the lock here: whoever takes it next finds this thread waiting
        return wait(*a)
    m._req_pool_lock.wait = waiting
    t = threading.Thread(target=lambda: got.append(m._acquire_llm()), daemon=True)
    t.start()
    assert asleep.wait(10)
    return t, got


def test_waiter_at_the_cap_is_woken_by_a_release_and_by_a_reload(model):
    m = model
    m.max_llm_requests = 1
    a = m._acquire_llm()
    t, got = _blocked_acquire(m)
    m._release_llm(a)
    t.join(10)
    assert got == [a]                  # by the release of a current pair
    t, got = _blocked_acquire(m)
    m._drop_contexts()
    t.join(10)
    assert len(got) == 1 and got[0][0] is not a[0] and m._req_made == 1   # by the reload: a pair of the new pool
    t, got2 = _blocked_acquire(m)
    m._release_llm(a)                  # stale: wakes the waiter, which finds nothing and sleeps again
    assert m._req_pool == [] and m._req_made == 1
    m._release_llm(got[0])
    t.join(10)
    assert got2 == got


# ------------------------------------------------------------------ streaming encoder caches
def _flow(cap=None):
    f = CausalMaskedDiffWithXvec(FlowConfig.tiny(), torch.bfloat16, "cpu")   # no weights: only its cache bookkeeping is used
    assert f.stream_cache_cap == 8 and len(f._stream_caches) == 0            # the default
    if cap is not None:
        f.stream_cache_cap = cap
    f.encoder = SimpleNamespace(new_stream_cache=lambda cap: SimpleNamespace(cap=cap))
    return f


def test_live_requests_keep_their_caches_under_churn():
    f = _flow()
    live = [f"live-{i}" for i in range(4)]         # max_llm_requests streaming requests, their chunk calls interleaved
    mine = {k: f._stream_cache(k, 100) for k in live}
    for rnd in range(40):
        for k in live:
            assert f._stream_cache(k, 100 + rnd) is mine[k]
        f._stream_cache(f"done-{rnd}", 100)        # a request that came and went ...
        if rnd % 3 == 0:
            f.drop_stream_cache(f"done-{rnd}")     # ... with or without its clean-up
        assert len(f._stream_caches) <= 8 and all(f._stream_caches[k] is mine[k] for k in live)


def test_eviction_is_least_recently_used_and_spares_the_call_in_progress():
    f = _flow(cap=3)
    a, b, c = (f._stream_cache(k, 10) for k in "abc")
    assert f._stream_cache("a", 10) is a           # renews a
    d = f._stream_cache("d", 10)
    assert list(f._stream_caches) == ["c", "a", "d"] and f._stream_caches["d"] is d
    big = f._stream_cache("c", 5000)               # outgrew its cache: a larger one, in its own place, nothing else evicted
    assert big is not c and big.cap >= 5000 and list(f._stream_caches) == ["a", "d", "c"]
    f.stream_cache_cap = 1
    e = f._stream_cache("e", 10)
    assert list(f._stream_caches) == ["e"] and f._stream_caches["e"] is e


def test_drop_beside_insert_raises_nothing():
    f = _flow(cap=4)
    errors = []

    def run(fn):
        try:
            for i in range(3000):
                fn(f"k{i % 16}")
        except BaseException as e:     # noqa: the test reports it
            errors.append(e)
    ts = [threading.Thread(target=run, args=(lambda k: f._stream_cache(k, 10),)), threading.Thread(target=run, args=(f.drop_stream_cache,))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errors and len(f._stream_caches) <= 4
