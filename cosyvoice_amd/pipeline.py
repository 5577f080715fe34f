"""The batch pipeline behind ``CosyVoice2Model.tts_batches``: the scheduling policy (plain bookkeeping: no device, no threads, no
streams; tests/test_pipeline_cpu.py), the CU-partitioned pipeline (one ``PartitionedPipeline`` per call) and the shared-CU one."""
import functools
import itertools
import queue
import threading
import time
from collections import deque
from concurrent.futures import Future, ThreadPoolExecutor
from typing import NamedTuple

import torch

FLOW_KEYS = ("flow_prompt_speech_tokens", "prompt_speech_feats", "flow_embeddings")


# ------------------------------------------------------------------ scheduling policy
class CuPartition(NamedTuple):
    """The CU-masked streams of ``CosyVoice2Model.cu_partition``."""
    llm: list        # one per concurrent decode loop, all on the decode CUs
    flow: object     # flow + HiFT, on the other CUs
    borrow: object   # a decode loop borrowing the idle flow CUs
    prefill: list    # prefills, on the flow CUs (one per decode loop)
    hift: object     # HiFT of batch i beside the flow of batch i + 1


def ragged_prompts(b):
    """A batch whose flow prompts are per-utterance lists (different lengths) instead of stacked (B, Np) / (B, Tp, 80) tensors."""
    return isinstance(b["flow_prompt_speech_tokens"], (list, tuple))


def same_layout(a, c):
    if ragged_prompts(a) or ragged_prompts(c):   # per-utterance prompt lists: such a batch is a flow pass of its own
        return False
    return all(a[k].shape[1:] == c[k].shape[1:] for k in FLOW_KEYS)


class Admission:
    """How many batches a decode job takes and when it may start: ``n_llm`` decode loops, ``merge`` batches per job at most (fewer
    while ``ramp`` lasts), ``max_batch`` rows per job."""

    def __init__(self, n_llm, merge, ramp, max_batch):
        self.merge, self.max_batch = max(1, int(merge)), max_batch
        self.cap = (max(1, n_llm) + 2) * self.merge   # batches in flight: n_llm decode loops busy plus one job queued behind them
        # pipeline fill: the first decode jobs are small so that the flow stream gets its first batches early and is then fed without a
        # gap while the job size grows to `merge` (1, 2, 2, 3, merge, ...: with 4 batches per job from the start the flow CUs idled ~0.2 s)
        self.ramp = [int(v) for v in ramp]
        self.n_jobs = 0   # decode jobs filled so far

    def job_size(self, n=None):
        n = self.n_jobs if n is None else n
        return min(self.merge, self.ramp[n]) if n < len(self.ramp) else self.merge

    def admits(self, k):
        """May the next job start with ``k`` batches in flight?  Only when ALL its batches fit: a job cut short by the in-flight cap (one
        batch in a 4-batch slot) occupies a decode loop for 70 % of a full job's time."""
        return k == 0 or k + self.job_size() <= self.cap

    def fill(self, nxt, draw):
        """The batches of the next job, from the looked-ahead batch ``nxt`` on (``draw()`` -> the batch after, or None) -> (job, new nxt)."""
        bs, rows, size = [], 0, self.job_size()
        while nxt is not None and len(bs) < size and rows + len(nxt["texts"]) <= self.max_batch:
            rows += len(nxt["texts"])
            bs.append(nxt)
            nxt = draw()
        if not bs:
            raise ValueError(f"a batch of {len(nxt['texts'])} utterances exceeds the LLM's max_batch {self.max_batch}")
        self.n_jobs += 1
        return bs, nxt


def depth(n_llm, merge):
    """The largest number of batches that hold their buffers at once.  ``n_llm`` decode loops on their CU share: the in-flight cap plus
    the one batch looked ahead; 0 (the shared-CU pipeline): the batch being decoded plus the one whose waveform is pending."""
    return Admission(n_llm, merge, (), 0).cap + 1 if n_llm else 2


def flow_group(head, q, fmerge):
    """``head`` (the oldest queued batch, already taken from ``q``: the flow thread has waited for its tokens) plus the batches right behind
    it whose tokens are ALREADY there, up to ``fmerge`` in all and of the same prompt lengths."""
    grp = [head]
    while (len(grp) < fmerge and q and q[0]["lf"].done() and q[0]["lf"].exception() is None
           and same_layout(head["b"], q[0]["b"])):
        grp.append(q.popleft())
    return grp


def split_rows(wav, counts, done):
    """result of a flow group -> one (wav, done) per batch of the group (rows in batch order)"""
    if isinstance(wav, list):   # ragged: per-utterance waveforms
        out, o = [], 0
        for c in counts:
            out.append((wav[o:o + c], done))
            o += c
        return out
    return [(w, done) for w in wav.split(counts, dim=0)] if len(counts) > 1 else [(wav, done)]


def consumer_copy(wav, to_host, stream):
    """A pass's waveforms as the consumer gets them -> (wav, done).  On the host (the D2H copy orders them behind the pass: ``done`` is
    None), or a copy of their own with the event ``done`` recorded behind it on ``stream``: the equal-length path returns a view of HiFT's
    per-shape workspace, which the next pass overwrites on this stream as soon as its tokens arrive."""
    ragged = isinstance(wav, list)
    if to_host:
        return ([w.cpu() for w in wav] if ragged else wav.cpu()), None
    wav = [w.clone() for w in wav] if ragged else wav.clone()
    done = torch.cuda.Event()
    done.record(stream)
    return wav, done


def merged_adapters(bs):
    """The optional per-utterance ``"llm_adapters"`` lists of the batches one decode job merges, concatenated in row order like their
    texts; None when no batch carries the key.  A merge in which only some batches carry it is refused: the rows of the others would
    silently fall to the base model or to a neighbour's voice."""
    have = [b.get("llm_adapters") is not None for b in bs]
    if not any(have):
        return None
    if not all(have):
        raise ValueError(f"llm_adapters is set on {sum(have)} of the {len(bs)} batches merged into one decode job: set it on all or none")
    for b in bs:
        if len(b["llm_adapters"]) != len(b["texts"]):
            raise ValueError(f"llm_adapters has {len(b['llm_adapters'])} entries for a batch of {len(b['texts'])} utterances")
    return [a for b in bs for a in b["llm_adapters"]]


def decode_job(ctx, bs, **kw):
    """One ``generate_batch`` of ``ctx`` over the utterances of the batches ``bs`` -> the token lists of each batch."""
    cat = lambda key: [x for b in bs for x in b[key]]
    forced = cat("forced") if all(b.get("forced") is not None for b in bs) else None
    adapters = merged_adapters(bs)
    if adapters is not None:
        kw["adapters"] = adapters
    toks = ctx.generate_batch(cat("texts"), cat("prompt_texts"), cat("llm_prompt_speech_tokens"), forced=forced, **kw)
    out, o = [], 0
    for b in bs:
        out.append(toks[o:o + len(b["texts"])])
        o += len(b["texts"])
    return out


def _call(b, name):
    if b.get(name) is not None:
        b[name]()


def _release(held):
    """The end of a run, however it ends (its host threads have ended): every batch that was drawn and whose waveform was not handed out
    (in flight, or looked ahead and never started) gets its ``on_done``, in batch order, once the device is done with their work."""
    try:
        if held:
            torch.cuda.synchronize()
    finally:
        while held:
            _call(held.popleft(), "on_done")


@torch.no_grad()
def shared_pipeline(model, batches, to_host):
    """Both stages on all CUs: the decode loop of batch i + 1 on the model's side stream beside flow + HiFT of batch i on the caller's."""
    llm_stream = model.llm_context.stream if hasattr(model.llm_context, "stream") else torch.cuda.Stream()
    pending, held = None, deque()
    try:
        for b in itertools.chain(batches, [None]):   # lazily: a batch takes its buffers when its turn comes
            toks = None
            if b is not None:
                held.append(b)
                with torch.cuda.stream(llm_stream):
                    _call(b, "on_start")
                    ready = torch.cuda.Event()
                    ready.record(llm_stream)
                    toks = decode_job(model.llm, [b])[0]
            if pending is not None:
                out, done = consumer_copy(pending, to_host, torch.cuda.current_stream())
                if done is not None:
                    done.synchronize()   # on_done promises that nothing reads the batch's inputs any more
                _call(held.popleft(), "on_done")
                yield out
                pending = None
            if toks is not None:
                torch.cuda.current_stream().wait_event(ready)  # conditioning of this batch is in place
                pending = model._flow_hift(b, toks)
    finally:
        _release(held)


# ------------------------------------------------------------------ the CU-partitioned pipeline
class PartitionedPipeline:
    """One ``tts_batches`` call with the decode loops on ``k`` CU slots of every XCD and flow + HiFT on the others: ``n_llm`` decode
    threads, the flow thread and (``overlap_hift``) the vocoder thread, fed and collected by the calling thread (``run``)."""

    def __init__(self, model, to_host, k, n_llm):
        self.model, self.to_host = model, to_host
        self.part = model.cu_partition(k, n_llm)
        self.est = model.flow.decoder.estimator
        self.budget = (32 - k) * 8   # the flow's launches run on that many CUs: its row-block kernels size their tiles for it
        self.flow_full = torch.cuda.Stream(model.device)   # all CUs: the last batch's flow + HiFT run after every decode loop ended
        self.caller = torch.cuda.current_stream()
        # Admission work (drawing a batch from ``batches``, its on_start, the `ready` event) runs on a private non-blocking stream, not on the
        # caller's: when that is the legacy default stream every operation on it — a conditioning copy, an event record — is an implicit barrier
        # against all the CU-masked streams of the pipeline (they are blocking streams), i.e. the whole pipeline drained once per admitted
        # batch (625 -> 638 audio-s/s at 20 passes, 639 -> 664 at 32, profiles/r03_flow_merge_sweeps.log).
        self.adm = torch.cuda.Stream(model.device)
        self.adm.wait_stream(self.caller)   # whatever the caller enqueued before the call is visible to the first batch
        self.ctxs = queue.Queue()
        for ctx in zip(model.llm_contexts(n_llm), self.part.llm, self.part.prefill):
            self.ctxs.put(ctx)
        self.n_llm, self.fmerge = n_llm, max(1, int(model.flow_merge))
        self.jobs = Admission(n_llm, model.llm_merge, model.llm_ramp, model.llm.max_batch)
        self.flow_q, self.flow_cv, self.closed, self.abort = deque(), threading.Condition(), False, False
        self.llm_lock, self.llm_running, self.all_submitted = threading.Lock(), 0, False
        self.drawn, self.inflight = deque(), deque()   # batches drawn and not yet handed out; of these, (batch, future) of the started ones

    def llm_job(self, bs, ready, borrow):
        """One decode job over the utterances of ``bs`` (``llm_merge`` consecutive batches share one token loop: the step
        is a weight stream, 16 rows cost 1.3x the time of 8) -> the token lists of each batch."""
        m = self.model
        ctx, own, pf = self.ctxs.get()
        try:
            # first batch of the run: the flow CUs are idle, decode there (more CUs, nothing to disturb)
            stream = self.part.borrow if borrow else own
            t_job = time.perf_counter()
            if merged_adapters(bs) is not None:
                m.sync_lora(ctx)
            with torch.no_grad(), torch.cuda.stream(stream):
                stream.wait_event(ready)   # inputs the caller produced / the conditioning broadcast
                # the prefill is throughput-bound GEMM work: it runs beside flow + HiFT on their (three times larger)
                # CU share, the decode partition only runs the token loop
                out = decode_job(ctx, bs, steps_per_poll=64, prefill_stream=None if (borrow or not m.prefill_on_flow_cus) else pf)
            if m.pipeline_stats is not None:   # generate_batch ends with a D2H of the token buffer: the loop is drained
                m.pipeline_stats.append(("llm", len(bs), t_job, time.perf_counter()))
            return out
        finally:
            self.ctxs.put((ctx, own, pf))
            with self.llm_lock:
                self.llm_running -= 1

    def result(self, wav, counts, stream, t_job):
        """The epilogue of a flow group: the consumer's copy of its waveforms, split per batch."""
        wav, done = consumer_copy(wav, self.to_host, stream)
        if self.to_host and self.model.pipeline_stats is not None:
            self.model.pipeline_stats.append(("flow", len(counts), t_job, time.perf_counter()))
        return split_rows(wav, counts, done)

    def hift_job(self, mel, lens, mel_ready, t_job, counts):
        """HiFT (+ D2H) of one flow group on its own stream over the flow CUs: the vocoder of group i fills the CUs the
        flow of group i + 1 leaves idle (the tail round of every attention launch, tile quantisation of the row-block
        kernels) instead of extending the flow stream's critical path (17 of a 91 ms job on all CUs).  ``lens``: frame counts of a
        ragged group (mel padded, one ragged vocoder pass) or None."""
        hift, hift_part = self.model.hift, self.part.hift
        with torch.no_grad(), torch.cuda.stream(hift_part):
            hift_part.wait_event(mel_ready)
            mel.record_stream(hift_part)
            if lens is None:
                wav, _ = hift.inference(speech_feat=mel, cache_source=torch.zeros(1, 1, 0))
            else:
                wav, _ = hift.inference_ragged(mel, lengths=lens)
            return self.result(wav, counts, hift_part, t_job)

    def flow_job(self, grp, stream):
        """Flow + HiFT of ``grp`` = consecutive batches whose tokens are ready (``flow_merge`` of them at most, same prompt lengths) as a single
        pass: the row-block kernels run in whole rounds of workgroups over the stream's CUs, so 16 or 24 utterances cost less per utterance
        than 8 (tools/flow_share_probe.py: 13.9 / 12.3 / 11.5 ms per utterance at 8 / 16 / 24 on the 192-CU share).  Every entry of ``grp``
        holds its batch, its decode job's future and its index in that job.  -> one (wav, done) per batch, or the vocoder job that gives them."""
        m = self.model
        per_b = [t["lf"].result()[t["idx"]] for t in grp]
        counts = [len(tb) for tb in per_b]
        toks = [t for tb in per_b for t in tb]
        ready_evs = {id(t["ready"]): t["ready"] for t in grp}.values()   # one per decode job
        t_job = time.perf_counter()
        with self.llm_lock:
            # every decode job of the run has ended and none is left to submit: the decode CUs are idle for good, so the remaining
            # flow + HiFT passes (the pipeline's drain: up to 2 x llm_merge batches) take all CUs, not only the last batch
            if self.llm_running == 0 and self.all_submitted:
                stream = self.flow_full
        # tile sizes of the row-block kernels (and the solver graph that bakes them in) follow the CUs of the stream
        self.est.cu_budget = 0 if stream is self.flow_full else self.budget
        equal = all(len(t) == len(toks[0]) for t in toks) and not ragged_prompts(grp[0]["b"])
        own_hift = m.overlap_hift and (equal or m.ragged_hift)   # the vocoder as a job of its own on the HiFT stream
        with torch.no_grad(), torch.cuda.stream(stream):
            for r in ready_evs:
                stream.wait_event(r)
            stream.wait_stream(self.part.flow if stream is self.flow_full else self.flow_full)  # workspaces of the previous group
            if m.overlap_hift and not own_hift:
                self.hift_pool.submit(lambda: None).result()   # earlier groups' vocoder jobs are enqueued ...
                stream.wait_stream(self.part.hift)             # ... and done with the vocoder workspaces before this one uses them
            # a merged group is concatenated here, on the job's stream behind `ready`: never on this thread's default stream
            b = grp[0]["b"] if len(grp) == 1 else {k: torch.cat([t["b"][k] for t in grp], dim=0) for k in FLOW_KEYS}
            if not own_hift:
                return self.result(m._flow_hift(b, toks), counts, stream, t_job)
            if equal:
                tok = torch.tensor(toks, dtype=torch.int32, device=m.device)
                mel = m.flow.inference_batch(tok, b["flow_prompt_speech_tokens"], b["prompt_speech_feats"], b["flow_embeddings"])
                mel, lens = mel.contiguous().clone(), None   # the flow's output buffer is rewritten by the next group
            else:
                mel, lens = m._flow_ragged(b, toks)          # a padded tensor of its own
            mel_ready = torch.cuda.Event()
            mel_ready.record(stream)
        return self.hift_pool.submit(self.hift_job, mel, lens, mel_ready, t_job, counts)   # one worker: vocoder workspaces are used in group order

    def flow_worker(self):
        """The flow thread: takes the oldest batch whose tokens it then waits for, adds the batches right behind it whose tokens are ALREADY
        there (``flow_group``) and runs them as one pass — groups form across decode jobs when the flow side has
        a backlog and never wait for tokens when it has none (the pipeline's fill)."""
        while True:
            with self.flow_cv:
                while not self.flow_q and not self.closed:
                    self.flow_cv.wait()
                if not self.flow_q:
                    return
                grp = [self.flow_q.popleft()]
            try:
                if self.abort:
                    raise RuntimeError("tts_batches closed before this batch was vocoded")
                grp[0]["lf"].result()
                with self.flow_cv:
                    grp = flow_group(grp[0], self.flow_q, self.fmerge)
                res = self.flow_job(grp, self.part.flow)
            except BaseException as e:
                for t in grp:
                    t["fut"].set_exception(e)
                continue
            if hasattr(res, "add_done_callback"):   # the equal-length overlap path hands back its vocoder job
                res.add_done_callback(functools.partial(self.deliver, grp))
            else:
                self.deliver(grp, res)

    def deliver(self, grp, r):
        try:
            for t, x in zip(grp, r.result() if hasattr(r, "result") else r):
                t["fut"].set_result(x)
        except BaseException as e:
            for t in grp:
                if not t["fut"].done():
                    t["fut"].set_exception(e)

    def collect(self, fut):
        wav, done = fut.result()
        if done is not None:   # to_host=False: the flow group's work is only enqueued
            self.caller.wait_event(done)
            done.synchronize()   # on_done promises that nothing reads the batch's inputs any more
        return wav

    def draw(self):
        with torch.cuda.stream(self.adm):
            b = next(self.it, None)
        if b is not None:
            self.drawn.append(b)
        return b

    def submit(self, bs, last):
        """Start the decode job of ``bs`` and queue its batches for the flow thread."""
        ready = torch.cuda.Event()
        with torch.cuda.stream(self.adm):
            for b in bs:
                _call(b, "on_start")   # e.g. the conditioning broadcast: same order on every rank, never from worker threads
            ready.record(self.adm)
        with self.llm_lock:
            self.llm_running += 1
            self.all_submitted = last
        lf = self.llm_pool.submit(self.llm_job, bs, ready, self.jobs.n_jobs == 1)
        with self.flow_cv:
            for i, b in enumerate(bs):
                t = dict(b=b, lf=lf, idx=i, ready=ready, fut=Future())
                self.flow_q.append(t)
                self.inflight.append((b, t["fut"]))
            self.flow_cv.notify()

    def schedule(self):
        nxt = self.draw()
        while nxt is not None or self.inflight:
            while nxt is not None and self.jobs.admits(len(self.inflight)):
                bs, nxt = self.jobs.fill(nxt, self.draw)
                self.submit(bs, nxt is None)
            b, fut = self.inflight.popleft()
            self.drawn.popleft()
            try:
                wav = self.collect(fut)
            finally:
                _call(b, "on_done")   # every job of this batch (decode, flow, vocoder) has ended: its conditioning slot is free
            yield wav

    def run(self, batches):
        self.it = iter(batches)
        try:
            self.est.cu_budget = self.budget
            # left in reverse order: the flow thread ends first (it needs the other two), then the decode jobs, then the vocoder jobs
            with ThreadPoolExecutor(max_workers=1) as self.hift_pool, ThreadPoolExecutor(max_workers=self.n_llm) as self.llm_pool, \
                    ThreadPoolExecutor(max_workers=1) as flow_pool:
                flow_pool.submit(self.flow_worker)
                try:
                    yield from self.schedule()
                finally:
                    with self.flow_cv:   # normal end: the queue is empty; a consumer that stopped early: the flow thread fails what is left instead of running it
                        self.closed, self.abort = True, bool(self.flow_q)
                        self.flow_cv.notify()
        finally:
            self.est.cu_budget = 0
            _release(self.drawn)
