"""Orchestrator — drop-in for the reference's ``CosyVoice2Model`` (/root/reference/cosyvoice/cli/model.py:295-424):
per-request uuid state, LLM producer thread (``llm_job``), ``token2wav`` (flow -> HiFT with the streaming
mel/source/speech caches and hamming cross-fade), ``tts`` generator yielding ``{'tts_speech': Tensor(1,S) cpu}``.

The stage objects are the HIP-backed ``cosyvoice_amd.llm.Qwen2LM`` / ``flow.CausalMaskedDiffWithXvec`` /
``hift.HiFTGenerator`` (they expose what the orchestrator touches, SURVEY.md §8b level 1), so
``cosyvoice.cli`` code that builds a CosyVoice2Model keeps working with this class.

``tts_batch`` is the build's utterance-batched entry (the reference is batch-1): LLM decode batched over B
sequences, flow batched over B CFG pairs, HiFT batched over B mels.
"""
import collections
import threading
import time
import uuid
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import pipeline
from .pipeline import CuPartition, ragged_prompts


def fade_in_out(fade_in_mel, fade_out_mel, window):
    """utils/common.py:149-157 (host-side cross-fade of the stream seam)."""
    device = fade_in_mel.device
    fade_in_mel, fade_out_mel = fade_in_mel.cpu().clone(), fade_out_mel.cpu()
    n = int(window.shape[0] / 2)
    w = torch.as_tensor(window)   # float64 hamming window, as the reference's numpy broadcast (result is cast back on assignment)
    fade_in_mel[..., :n] = fade_in_mel[..., :n] * w[:n] + fade_out_mel[..., -n:] * w[n:]
    return fade_in_mel.to(device)


class CosyVoice2Model:
    def __init__(self, llm, flow, hift, fp16: bool = False):
        self.device = torch.device("cuda")
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.llm, self.flow, self.hift = llm, flow, hift
        self.fp16 = fp16
        self.llm.fp16 = fp16
        self.flow.fp16 = fp16
        self.token_hop_len = 2 * self.flow.input_frame_rate
        # model.py:313-315
        if hasattr(self.flow, "token_mel_ratio"):     # CosyVoice2 flow; the v1 MaskedDiffWithXvec has no chunk attention
            self.flow.encoder.static_chunk_size = 2 * self.flow.input_frame_rate
            self.flow.decoder.estimator.static_chunk_size = 2 * self.flow.input_frame_rate * self.flow.token_mel_ratio
        self.mel_cache_len = 8
        self.source_cache_len = int(self.mel_cache_len * 480)
        self.speech_window = np.hamming(2 * self.source_cache_len)
        self.stream_scale_factor = 1
        # high-priority side stream: the decode loop is a chain of short dependent kernels that must not queue behind the
        # flow GEMMs of the previous batch when both streams are busy (tts_batches)
        self.llm_context = torch.cuda.stream(torch.cuda.Stream(self.device, priority=-1))
        # streaming requests run the flow at the next multiple of this many tokens (tail masked, exact): requests of arbitrary
        # prompt / chunk lengths then share a handful of captured estimator graphs instead of capturing one per length
        self.stream_length_bucket = 25
        self.llm_cu_slots = 8   # tts_batches: CU slots per XCD (of 32) owned by the decode loops; 0 = no partition
        self.llm_loops = 2      # tts_batches: concurrent decode loops (each its own batch / KV caches) on those CUs
        self.llm_merge = 1      # tts_batches: consecutive batches decoded by ONE token loop (rows <= llm.max_batch)
        self.flow_merge = 1     # tts_batches: up to this many consecutive batches whose tokens are ready share ONE flow + HiFT pass
        self.llm_ramp = (1, 2, 2, 3)   # tts_batches: batches per decode job while the pipeline fills (then llm_merge)
        self.lock = threading.Lock()
        # The reference's modules are re-entrant (every call builds its own activations / KV cache) and it interleaves requests:
        # one LLM thread + side stream per tts() call (cli/model.py:62,119,189).  Here a decode loop owns KV caches, device state and
        # captured graphs, so every request takes its OWN decode context over the one set of weights (Qwen2LM.new_context) from a
        # pool of ``max_llm_requests`` and runs it on that context's stream: the token loops of concurrent requests overlap.  The
        # flow / vocoder objects keep one workspace set: token2wav calls take turns (flow_lock) — they are GPU-bound, not
        # latency-bound, so nothing is gained by interleaving them (batches go through tts_batch / tts_batches instead).
        self.max_llm_requests = 4
        self.llm_lock = threading.Lock()          # only for LMs without decode contexts (the v1 TransformerLM)
        self._req_pool_lock = threading.Condition()
        self._req_pool = []                       # [(context, stream)] free for requests
        self._req_made = 0                        # pairs made since the last reset (free or in use), <= max_llm_requests
        self._req_gen = 0                         # counts the resets (_drop_contexts): a pair of an earlier one is stale
        self.flow_lock = threading.Lock()
        self.tts_speech_token_dict = {}
        self.llm_end_dict = {}
        self.hift_cache_dict = {}
        self._llm_spans = collections.OrderedDict()   # uuid -> [start, end] wall-clock of the request's token loop (diagnostics / tests); the last 64 requests
        self._llm_errors = {}     # uuid -> exception raised inside the request's LLM thread; tts() re-raises it in the caller
        self.overlap_hift = False   # tts_batches: HiFT of batch i on its own stream beside flow of batch i + 1 (measured SLOWER: 455 vs 548 audio-s/s — the vocoder GEMMs and the flow chain disturb each other on shared CUs; kept for experiments)
        # tts_batches: where the decode jobs' prefills run.  True = on the flow CUs (throughput-bound GEMM work over B x 282 rows); False = on
        # the decode CUs with the token loop.  Re-checked in round 2, when the flow + HiFT stream became the bottleneck: still better on the
        # flow CUs (622-631 vs 605-612 audio-s/s) — on 64 CUs a 32-row prefill stalls both token loops for ~0.1 s per job
        self.prefill_on_flow_cus = True
        self.pipeline_stats = None  # set to a list to collect (stage, batches, start, end) of every tts_batches job
        # utterances of different generated lengths (free-running sampling): True = ONE ragged vocoder pass over the padded batch
        # (HiFTGenerator.inference_ragged, exact per utterance); False = the per-utterance loop of batch-1 vocoder calls, kept as the cross-check
        self.ragged_hift = True

    def _drop_contexts(self):
        """Forget every extra decode context (they share the weight tensors of the LM they were made from: after a reload they
        would keep decoding with the old weights) and their captured graphs."""
        from . import ops
        with self._req_pool_lock:
            ctxs = [c for c, _ in self._req_pool] + [c for c in (getattr(self, "_llm_contexts", None) or []) if c is not self.llm]
            for c in ctxs:
                ops.drop_graphs(getattr(c, "_graphs", {}))
            # pairs that requests still hold belong to the generation that ends here: _release_llm discards them
            self._req_pool, self._req_made, self._req_gen = [], 0, self._req_gen + 1
            self._llm_contexts = None
            self._req_pool_lock.notify_all()      # requests waiting at the cap may make pairs of the new generation

    def load(self, llm_model, flow_model, hift_model):
        """model.py:71-81 — three flat state-dict files with the reference key names."""
        self._drop_contexts()
        self.llm.load_state_dict(torch.load(llm_model, map_location="cpu", weights_only=True), strict=False)
        self.flow.load_state_dict(torch.load(flow_model, map_location="cpu", weights_only=True), strict=False)
        hift_sd = {k.replace("generator.", ""): v for k, v in torch.load(hift_model, map_location="cpu", weights_only=True).items()}
        self.hift.load_state_dict(hift_sd, strict=False)

    def load_state_dicts(self, llm_sd, flow_sd, hift_sd):
        self._drop_contexts()
        self.llm.load_state_dict(llm_sd)
        self.flow.load_state_dict(flow_sd)
        self.hift.load_state_dict(hift_sd)
        return self

    def _acquire_llm(self):
        """A free (decode context, stream) pair for one request; grows the pool up to max_llm_requests, then waits.  Every pooled
        context is a Qwen2LM.new_context(): ``self.llm`` itself stays reserved for the batch paths (tts_batch / tts_batches use it
        without taking the pool), so a tts() request never shares KV caches or device state with a running batch."""
        with self._req_pool_lock:
            while True:
                if self._req_pool:
                    return self._req_pool.pop()
                if self._req_made < self.max_llm_requests:
                    self._req_made += 1
                    gen = self._req_gen
                    break
                self._req_pool_lock.wait()
        ctx = self.llm.new_context()
        ctx._pool_gen = gen
        return ctx, torch.cuda.Stream(self.device, priority=-1)

    def _release_llm(self, pair):
        """Back into the pool — unless the pair was taken before a reload (_drop_contexts): its context shares the OLD weight
        tensors, so it is discarded with its captured graphs and counts for nothing in the pool that replaced its own."""
        with self._req_pool_lock:
            stale = pair[0]._pool_gen != self._req_gen
            if not stale:
                self._req_pool.append(pair)
            self._req_pool_lock.notify()
        if stale:
            from . import ops
            ops.drop_graphs(getattr(pair[0], "_graphs", {}))

    def sync_lora(self, ctx):
        """A decode context made before ``self.llm.attach_lora(bank)`` (or before the bank was replaced) takes the LM's current bank."""
        mine = getattr(self.llm, "_lora", None)
        if mine is not None and (ctx._lora is None or ctx._lora["bank"] is not mine["bank"]):
            ctx.attach_lora(mine["bank"])
        return ctx

    def llm_job(self, text, prompt_text, llm_prompt_speech_token, llm_embedding, uuid_, seed=None, lora=None):
        # model.py:116-128.  The fork's phoneme LMs (Qwen2LM_Phoneme_Src2.inference, llm.py:1687-1699) take
        # text = (bpe ids, phoneme factors) and matching length tuples: tuples are passed through in that form.
        dev = self.device
        if isinstance(text, (tuple, list)):
            to = lambda t: tuple(x.to(dev) for x in t)
            ln = lambda t: tuple(torch.tensor([x.shape[1]], dtype=torch.int32) for x in t)
            text_a, text_len, ptext_a, ptext_len = to(text), ln(text), to(prompt_text), ln(prompt_text)
        else:
            text_a, text_len = text.to(dev), torch.tensor([text.shape[1]], dtype=torch.int32)
            ptext_a, ptext_len = prompt_text.to(dev), torch.tensor([prompt_text.shape[1]], dtype=torch.int32)
        kw = dict(text=text_a, text_len=text_len, prompt_text=ptext_a, prompt_text_len=ptext_len,
                  prompt_speech_token=llm_prompt_speech_token.to(self.device),
                  prompt_speech_token_len=torch.tensor([llm_prompt_speech_token.shape[1]], dtype=torch.int32), embedding=llm_embedding)
        if lora is not None:   # the request's LoRA adapter (a name or slot of the bank attached to self.llm, -1 = base model)
            kw["adapters"] = [lora]
        try:
            if hasattr(self.llm, "new_context"):
                pair = self._acquire_llm()
                try:
                    ctx, stream = pair
                    if lora is not None:
                        self.sync_lora(ctx)
                    with self.lock:
                        self._llm_spans[uuid_] = [time.perf_counter(), None]
                        while len(self._llm_spans) > 64:
                            self._llm_spans.popitem(last=False)
                    span = self._llm_spans[uuid_]
                    with torch.cuda.stream(stream):
                        for i in ctx.inference(nonce=seed, **kw):
                            self.tts_speech_token_dict[uuid_].append(i)
                        stream.synchronize()
                    span[1] = time.perf_counter()
                finally:
                    self._release_llm(pair)
            else:
                with self.llm_lock, self.llm_context:
                    for i in self.llm.inference(**kw):
                        self.tts_speech_token_dict[uuid_].append(i)
        except BaseException as e:      # the consumer loop of tts() polls llm_end_dict: it must see the end, and the error
            self._llm_errors[uuid_] = e
        finally:
            self.llm_end_dict[uuid_] = True

    def token2wav(self, *args, **kwargs):
        """Reference signature (model.py:334 / :130 for the v1 wiring); one call at a time per model object (flow_lock)."""
        with self.flow_lock:
            return self._token2wav(*args, **kwargs)

    def _token2wav(self, token, prompt_token, prompt_feat, embedding, uuid_, token_offset, finalize=False, speed=1.0):
        # model.py:334-366
        tts_mel, _ = self.flow.inference(token=token.to(self.device),
                                         token_len=torch.tensor([token.shape[1]], dtype=torch.int32),
                                         prompt_token=prompt_token.to(self.device),
                                         prompt_token_len=torch.tensor([prompt_token.shape[1]], dtype=torch.int32),
                                         prompt_feat=prompt_feat.to(self.device),
                                         prompt_feat_len=torch.tensor([prompt_feat.shape[1]], dtype=torch.int32),
                                         embedding=embedding.to(self.device), finalize=finalize,
                                         # a streaming request's chunk calls share its chunk-causal encoder state
                                         **({"cache_key": uuid_} if (getattr(self.flow, "supports_stream_cache", False)
                                                                     and (not finalize or token_offset > 0)) else {}))
        tts_mel = tts_mel[:, :, token_offset * self.flow.token_mel_ratio:]
        if self.hift_cache_dict[uuid_] is not None:
            hift_cache_mel, hift_cache_source = self.hift_cache_dict[uuid_]["mel"], self.hift_cache_dict[uuid_]["source"]
            tts_mel = torch.concat([hift_cache_mel, tts_mel], dim=2)
        else:
            hift_cache_source = torch.zeros(1, 1, 0)
        if finalize is False:
            tts_speech, tts_source = self.hift.inference(speech_feat=tts_mel, cache_source=hift_cache_source)
            tts_speech, tts_source = tts_speech.clone(), tts_source.clone()
            if self.hift_cache_dict[uuid_] is not None:
                tts_speech = fade_in_out(tts_speech, self.hift_cache_dict[uuid_]["speech"], self.speech_window)
            self.hift_cache_dict[uuid_] = {"mel": tts_mel[:, :, -self.mel_cache_len:].clone(),
                                           "source": tts_source[:, :, -self.source_cache_len:].clone(),
                                           "speech": tts_speech[:, -self.source_cache_len:].clone()}
            tts_speech = tts_speech[:, :-self.source_cache_len]
        else:
            if speed != 1.0:
                assert self.hift_cache_dict[uuid_] is None, "speed change only support non-stream inference mode"
                tts_mel = F.interpolate(tts_mel, size=int(tts_mel.shape[2] / speed), mode="linear")
            tts_speech, tts_source = self.hift.inference(speech_feat=tts_mel, cache_source=hift_cache_source)
            tts_speech = tts_speech.clone()
            if self.hift_cache_dict[uuid_] is not None:
                tts_speech = fade_in_out(tts_speech, self.hift_cache_dict[uuid_]["speech"], self.speech_window)
        return tts_speech

    def tts(self, text, flow_embedding, llm_embedding=torch.zeros(0, 192), prompt_text=torch.zeros(1, 0, dtype=torch.int32),
            llm_prompt_speech_token=torch.zeros(1, 0, dtype=torch.int32), flow_prompt_speech_token=torch.zeros(1, 0, dtype=torch.int32),
            prompt_speech_feat=torch.zeros(1, 0, 80), stream=False, speed=1.0, lora=None, **kwargs):
        # model.py:368-424.  ``lora`` (extra keyword): this request's LoRA adapter of the bank attached to the LLM (name, slot, -1 = base)
        this_uuid = str(uuid.uuid1())
        with self.lock:
            self.tts_speech_token_dict[this_uuid], self.llm_end_dict[this_uuid] = [], False
            self.hift_cache_dict[this_uuid] = None
        # ``seed`` (extra keyword, absent from the reference): Philox key material of this request's sampler; None draws it from
        # torch's global generator (as the reference samples from the global RNG), an int makes the request reproducible
        p = threading.Thread(target=self.llm_job, args=(text, prompt_text, llm_prompt_speech_token, llm_embedding, this_uuid, kwargs.get("seed")),
                             kwargs={} if lora is None else {"lora": lora})
        p.start()

        def check_llm():
            err = self._llm_errors.pop(this_uuid, None)
            if err is not None:
                raise err

        try:
            if stream is True:
                self.flow.length_bucket = self.stream_length_bucket
                if getattr(self.flow, "supports_stream_cache", False):   # room for the encoder caches of all requests in flight
                    self.flow.stream_cache_cap = max(self.flow.stream_cache_cap, self.max_llm_requests)
                token_offset = 0
                need = self.token_hop_len + self.flow.pre_lookahead_len
                while True:
                    time.sleep(0.02)
                    if len(self.tts_speech_token_dict[this_uuid]) - token_offset >= need:
                        this_tok = torch.tensor(self.tts_speech_token_dict[this_uuid][:token_offset + need]).unsqueeze(dim=0)
                        this_speech = self.token2wav(token=this_tok, prompt_token=flow_prompt_speech_token, prompt_feat=prompt_speech_feat,
                                                     embedding=flow_embedding, uuid_=this_uuid, token_offset=token_offset, finalize=False)
                        token_offset += self.token_hop_len
                        yield {"tts_speech": this_speech.cpu()}
                    if self.llm_end_dict[this_uuid] is True and len(self.tts_speech_token_dict[this_uuid]) - token_offset < need:
                        break
                p.join()
                check_llm()
                this_tok = torch.tensor(self.tts_speech_token_dict[this_uuid]).unsqueeze(dim=0)
                this_speech = self.token2wav(token=this_tok, prompt_token=flow_prompt_speech_token, prompt_feat=prompt_speech_feat,
                                             embedding=flow_embedding, uuid_=this_uuid, token_offset=token_offset, finalize=True)
                yield {"tts_speech": this_speech.cpu()}
            else:
                p.join()
                check_llm()
                this_tok = torch.tensor(self.tts_speech_token_dict[this_uuid]).unsqueeze(dim=0)
                this_speech = self.token2wav(token=this_tok, prompt_token=flow_prompt_speech_token, prompt_feat=prompt_speech_feat,
                                             embedding=flow_embedding, uuid_=this_uuid, token_offset=0, finalize=True, speed=speed)
                yield {"tts_speech": this_speech.cpu()}
        finally:
            p.join()
            with self.lock:
                self.tts_speech_token_dict.pop(this_uuid, None)
                self.llm_end_dict.pop(this_uuid, None)
                self.hift_cache_dict.pop(this_uuid, None)
                self._llm_errors.pop(this_uuid, None)
            if getattr(self.flow, "supports_stream_cache", False):
                self.flow.drop_stream_cache(this_uuid)

    # ------------------------------------------------------------------ utterance-batched path (beyond the reference)
    @torch.no_grad()
    def tts_batch(self, texts: List[torch.Tensor], prompt_texts: List[torch.Tensor], llm_prompt_speech_tokens: List[torch.Tensor],
                  flow_prompt_speech_tokens: torch.Tensor, prompt_speech_feats: torch.Tensor, flow_embeddings: torch.Tensor,
                  forced: Optional[List[List[int]]] = None, to_host: bool = True, adapters=None):
        """B utterances (texts / prompts of any lengths) through LLM -> flow -> HiFT.  Returns wav (B,S) when all sequences
        generated the same number of tokens (teacher-forced), else a list of B waveforms.  ``flow_prompt_speech_tokens`` /
        ``prompt_speech_feats`` may be lists of per-utterance (Np_b,) / (2 * Np_b, 80) tensors (prompts of different lengths): the
        result is then always a list.  ``adapters``: per utterance a LoRA adapter of the bank attached to the LLM (Qwen2LM.generate_batch)."""
        toks = self.llm.generate_batch(texts, prompt_texts, llm_prompt_speech_tokens, forced=forced,
                                       **({} if adapters is None else {"adapters": adapters}))
        wav = self._flow_hift(dict(flow_prompt_speech_tokens=flow_prompt_speech_tokens, prompt_speech_feats=prompt_speech_feats,
                                   flow_embeddings=flow_embeddings), toks)
        if isinstance(wav, list):   # sequences of different generated lengths
            return [w.cpu() for w in wav] if to_host else wav
        return wav.cpu() if to_host else wav.clone()   # never hand out a view of HiFT's per-shape workspace

    def cu_partition(self, llm_cu_slots: int, n_llm: int = 1):
        """``pipeline.CuPartition``: CU-masked streams giving the decode loop(s) ``llm_cu_slots`` of the 32 CUs of every XCD
        (one stream per concurrent decode loop, all on the same CUs) and flow + HiFT the rest (cached).  With both stages
        free to use all 256 CUs the decode step's short dependent kernels queue behind — and share CUs with — the flow
        GEMMs and run 1.6x slower while the two overlap (226 -> 368 ms per batch, tools/cumask_probe2.py); on disjoint CU
        sets neither disturbs the other."""
        from . import ops
        key = (llm_cu_slots, n_llm)
        if getattr(self, "_cu_partition_key", None) != key:
            self._release_partition()   # the previous split's streams are destroyed, not leaked
            k = llm_cu_slots
            flow_cus = lambda: ops.masked_stream(lambda s, x: s >= k)
            self._cu_partition = CuPartition(llm=[ops.masked_stream(lambda s, x: s < k) for _ in range(n_llm)], flow=flow_cus(),
                                             borrow=flow_cus(), prefill=[flow_cus() for _ in range(n_llm)], hift=flow_cus())
            self._cu_partition_key = key
        return self._cu_partition

    def _release_partition(self):
        from . import ops
        part = getattr(self, "_cu_partition", None)
        if part is not None:
            torch.cuda.synchronize()
            for field in part:
                for st in (field if isinstance(field, list) else [field]):
                    ops.destroy_masked_stream(st)
        self._cu_partition, self._cu_partition_key = None, None

    def close(self):
        """Release what this model holds inside the HIP runtime (captured graphs of every stage / decode context, CU-masked
        streams) while the runtime is alive.  The model stays usable: graphs and streams are rebuilt on demand."""
        torch.cuda.synchronize()
        req_ctxs = [c for c, _ in (self._req_pool or [])]
        for ctx in list(getattr(self, "_llm_contexts", None) or [self.llm]) + req_ctxs:
            for g in getattr(ctx, "_graphs", {}).values():
                g.destroy()
            getattr(ctx, "_graphs", {}).clear()
        dec = getattr(self.flow, "decoder", None)
        for g in getattr(dec, "_graphs", {}).values():
            g.destroy()
        getattr(dec, "_graphs", {}).clear()
        self._release_partition()

    def llm_contexts(self, n: int):
        """``n`` decode contexts over the one set of LLM weights (Qwen2LM.new_context)."""
        ctxs = getattr(self, "_llm_contexts", None)
        if ctxs is None or ctxs[0] is not self.llm:
            ctxs = [self.llm]
        while len(ctxs) < n:
            ctxs.append(self.llm.new_context())
        self._llm_contexts = ctxs
        return ctxs[:n]

    @torch.no_grad()
    def warm_pipeline_shapes(self, b, n_tokens: int, llm_cu_slots: Optional[int] = None, llm_loops: Optional[int] = None):
        """Set-up, not work: run every shape the partitioned pipeline of ``tts_batches`` can meet once — each decode context at 1 ..
        ``llm_merge`` batches of rows (prefill workspace + the captured step graph of that row count), flow + HiFT at 1 .. ``flow_merge``
        batches on the flow CUs and on all CUs (the drain) — so that no graph capture or workspace allocation lands inside a run.
        ``b``: one batch dict as given to ``tts_batches`` (its ``forced`` lists, if any, are used for the two decode steps)."""
        k = self.llm_cu_slots if llm_cu_slots is None else llm_cu_slots
        n_llm = max(1, self.llm_loops if llm_loops is None else llm_loops)
        if not k:
            return
        part = self.cu_partition(k, n_llm)
        B = len(b["texts"])
        forced = b.get("forced")
        for ctx, st, pf in zip(self.llm_contexts(n_llm), part.llm, part.prefill):
            for j in range(1, max(1, int(self.llm_merge)) + 1):
                if j * B > self.llm.max_batch:
                    break
                with torch.cuda.stream(st):
                    ctx.generate_batch(b["texts"] * j, b["prompt_texts"] * j, b["llm_prompt_speech_tokens"] * j,
                                       forced=None if forced is None else [list(t) for t in forced] * j, steps_per_poll=64, max_steps=2,
                                       prefill_stream=pf if self.prefill_on_flow_cus else None)
        est = self.flow.decoder.estimator
        flow_full = torch.cuda.Stream(self.device)
        zero = torch.zeros(1, 1, 0)
        for budget, stream in (((32 - k) * 8, part.flow), (0, flow_full)):
            est.cu_budget = budget
            for j in range(1, max(1, int(self.flow_merge)) + 1):
                rep = lambda t: torch.cat([t] * j, dim=0)
                tok = torch.randint(0, self.flow.cfg.vocab_size, (j * B, n_tokens), dtype=torch.int32).to(self.device)
                with torch.cuda.stream(stream):
                    mel = self.flow.inference_batch(tok, rep(b["flow_prompt_speech_tokens"]), rep(b["prompt_speech_feats"]),
                                                    rep(b["flow_embeddings"])).contiguous().clone()
                stream.synchronize()
                with torch.cuda.stream(part.hift):
                    self.hift.inference(speech_feat=mel, cache_source=zero)
                part.hift.synchronize()
        est.cu_budget = 0
        torch.cuda.synchronize()

    def tts_batches(self, batches, to_host: bool = True, llm_cu_slots: Optional[int] = None, llm_loops: Optional[int] = None):
        """Generator over a list of utterance batches (each a dict of tts_batch's arguments), software-pipelined the way
        the reference overlaps its LLM thread with flow/HiFT (cli/model.py:62,119,189): the LLM decode of later batches
        (latency-bound) runs while flow + HiFT of batch i (throughput-bound GEMMs) execute.  A batch may carry ``on_start``
        (callable, e.g. the RCCL conditioning broadcast; called from the calling thread, in batch order) and ``on_done`` (callable,
        called from the calling thread once the batch's result has been collected, i.e. when no job reads its inputs any more:
        where a pipelined caller recycles the batch's conditioning buffer, cosyvoice_amd.dist.ConditioningRing).  ``batches`` may be
        a generator: a batch is taken from it (and may acquire its buffers) only when the pipeline admits it.  On the partitioned path the generator and
        ``on_start`` run with a private non-blocking stream current (ordered behind everything the caller enqueued before the call): GPU work they issue
        through torch is ordered before the batch's jobs without touching the caller's stream.

        ``llm_cu_slots`` (default ``self.llm_cu_slots``) > 0 partitions the GPU: the decode loops run on that many CUs
        of every XCD and flow + HiFT on the others, each from its own host thread, every captured graph replayed launch by
        launch (``ops.Graph.launch`` on a masked stream).  ``llm_loops`` (default ``self.llm_loops``) decode loops run
        concurrently on the decode CUs, each on its own batch with its own KV caches: a decode step is a chain of 124 short
        latency-bound kernels, and two interleaved chains deliver 1.5x the tokens per second of one.
        ``flow_merge`` > 1: the flow thread runs the oldest batch together with up to ``flow_merge`` - 1 batches right behind it whose tokens are
        already there as ONE flow + vocoder pass (same mel per utterance: the flow is batch-invariant; rows come back to their batches in order).
        ``llm_cu_slots=0`` keeps both stages on all CUs (two plain streams, one decode loop, no merging)."""
        k = self.llm_cu_slots if llm_cu_slots is None else llm_cu_slots
        n = self.llm_loops if llm_loops is None else llm_loops
        if k:
            yield from pipeline.PartitionedPipeline(self, to_host, k, max(1, n)).run(batches)
        else:
            yield from pipeline.shared_pipeline(self, batches, to_host)

    def tts_batches_depth(self, llm_cu_slots: Optional[int] = None, llm_loops: Optional[int] = None) -> int:
        """The largest number of batches ``tts_batches`` keeps between taking them from ``batches`` and their ``on_done``: what a ring
        of per-batch buffers (cosyvoice_amd.dist.ConditioningRing) has to hold."""
        k = self.llm_cu_slots if llm_cu_slots is None else llm_cu_slots
        n = self.llm_loops if llm_loops is None else llm_loops
        return pipeline.depth(max(1, n) if k else 0, self.llm_merge)

    def _flow_hift(self, b, toks):
        """Flow + HiFT of one batch.  Equal generated lengths (teacher-forced runs, the benchmark): one batched pass ->
        wav (B, S).  Free-running sampling ends every sequence at its own step: the flow and the vocoder then each run once over
        the ragged batch (rows padded to the longest, every stage bounded by the row's own length: exact per utterance) -> list of
        B waveforms (S_b,).  ``ragged_hift = False``: the vocoder runs per utterance instead (the cross-check).  Prompts of different
        lengths (``flow_prompt_speech_tokens`` / ``prompt_speech_feats`` given as per-utterance lists, frontend.PromptFrontEnd.batch)
        take the ragged path whatever the generated lengths."""
        n = len(toks[0])
        zero = torch.zeros(1, 1, 0)
        if all(len(t) == n for t in toks) and not ragged_prompts(b):
            tok = torch.tensor(toks, dtype=torch.int32, device=self.device)
            mel = self.flow.inference_batch(tok, b["flow_prompt_speech_tokens"], b["prompt_speech_feats"], b["flow_embeddings"])
            wav, _ = self.hift.inference(speech_feat=mel.contiguous(), cache_source=zero)
            return wav
        B = len(toks)
        if self.ragged_hift:
            mel, lens = self._flow_ragged(b, toks)
            wavs, _ = self.hift.inference_ragged(mel, lengths=lens)
            return [w.clone() for w in wavs]   # never hand out views of HiFT's per-shape workspace
        mels = self.flow.inference_ragged([torch.tensor(t, dtype=torch.int32) for t in toks],
                                          [b["flow_prompt_speech_tokens"][i] for i in range(B)],
                                          [b["prompt_speech_feats"][i] for i in range(B)], b["flow_embeddings"])
        outs = []
        for mel in mels:
            wav, _ = self.hift.inference(speech_feat=mel.unsqueeze(0).contiguous(), cache_source=zero)
            outs.append(wav[0].clone())
        return outs

    def _flow_ragged(self, b, toks):
        """One flow pass over utterances of different generated lengths -> (padded left-aligned mel (B, 80, T) of its own, frame counts)."""
        B = len(toks)
        return self.flow.inference_ragged([torch.tensor(t, dtype=torch.int32) for t in toks],
                                          [b["flow_prompt_speech_tokens"][i] for i in range(B)],
                                          [b["prompt_speech_feats"][i] for i in range(B)], b["flow_embeddings"], padded=True)


class CosyVoiceModel(CosyVoice2Model):
    """Drop-in for the reference's ``CosyVoiceModel`` (/root/reference/cosyvoice/cli/model.py:27-292) — the v1 wiring, which
    the fork also drives CosyVoice2 modules with (bin/inference_online_codec.py): the estimator attends over the whole
    sequence (``static_chunk_size = 0``, :49-50; the encoder's chunk size is left alone), streaming works on hop-sized
    token windows with ``token_overlap_len`` = 20 tokens of overlap (every chunk sees only the prompt and its own window, the
    consumed tokens are dropped), consecutive mels are cross-faded over ``mel_overlap_len`` frames and the vocoder keeps a
    20-frame mel / source / speech cache (:52-60, :130-172).  ``vc`` feeds source speech tokens instead of running the LLM."""

    def __init__(self, llm, flow, hift, fp16: bool = False, sr: int = 22050):
        super().__init__(llm, flow, hift, fp16)
        self.sample_rate = sr
        self.flow.encoder.static_chunk_size = 0              # CosyVoice2Model.__init__ set 2 * frame rate; v1 never does
        self.flow.decoder.estimator.static_chunk_size = 0    # model.py:49-50
        self.token_min_hop_len = 2 * self.flow.input_frame_rate
        self.token_max_hop_len = 4 * self.flow.input_frame_rate
        self.token_overlap_len = 20
        self.mel_overlap_len = int(self.token_overlap_len / self.flow.input_frame_rate * sr / 256)
        self.mel_window = np.hamming(2 * self.mel_overlap_len)
        self.mel_cache_len = 20
        self.source_cache_len = int(self.mel_cache_len * 256)
        self.speech_window = np.hamming(2 * self.source_cache_len)
        self.mel_overlap_dict = {}
        self.flow_cache_dict = {}

    def _token2wav(self, token, prompt_token=torch.zeros(1, 0, dtype=torch.int32), prompt_feat=torch.zeros(1, 0, 80),
                  embedding=torch.zeros(0, 512), uuid_="0", finalize=False, speed=1.0):
        # model.py:130-172
        n = lambda t: torch.tensor([t.shape[1]], dtype=torch.int32)
        mel, self.flow_cache_dict[uuid_] = self.flow.inference(
            token=token.to(self.device), token_len=n(token), prompt_token=prompt_token.to(self.device), prompt_token_len=n(prompt_token),
            prompt_feat=prompt_feat.to(self.device), prompt_feat_len=n(prompt_feat), embedding=embedding.to(self.device),
            flow_cache=self.flow_cache_dict[uuid_], sample_rate=self.sample_rate)
        if self.mel_overlap_dict[uuid_].shape[2] != 0:
            mel = fade_in_out(mel, self.mel_overlap_dict[uuid_], self.mel_window)
        cache = self.hift_cache_dict[uuid_]
        cache_source = torch.zeros(1, 1, 0)
        if cache is not None:
            mel = torch.concat([cache["mel"], mel], dim=2)
            cache_source = cache["source"]
        if not finalize:
            self.mel_overlap_dict[uuid_] = mel[:, :, -self.mel_overlap_len:].clone()
            mel = mel[:, :, :-self.mel_overlap_len]
            speech, source = self.hift.inference(speech_feat=mel, cache_source=cache_source)
            speech, source = speech.clone(), source.clone()
            if cache is not None:
                speech = fade_in_out(speech, cache["speech"], self.speech_window)
            self.hift_cache_dict[uuid_] = {"mel": mel[:, :, -self.mel_cache_len:].clone(),
                                           "source": source[:, :, -self.source_cache_len:].clone(),
                                           "speech": speech[:, -self.source_cache_len:].clone()}
            return speech[:, :-self.source_cache_len]
        if speed != 1.0:
            assert cache is None, "speed change only support non-stream inference mode"
            mel = F.interpolate(mel, size=int(mel.shape[2] / speed), mode="linear")
        speech, _ = self.hift.inference(speech_feat=mel, cache_source=cache_source)
        speech = speech.clone()
        if cache is not None:
            speech = fade_in_out(speech, cache["speech"], self.speech_window)
        return speech

    def _open(self, uuid_, tokens, ended):
        with self.lock:
            self.tts_speech_token_dict[uuid_], self.llm_end_dict[uuid_] = tokens, ended
            self.hift_cache_dict[uuid_] = None
            self.mel_overlap_dict[uuid_] = torch.zeros(1, 80, 0)
            self.flow_cache_dict[uuid_] = torch.zeros(1, 80, 0, 2)

    def _close(self, uuid_):
        with self.lock:
            for d in (self.tts_speech_token_dict, self.llm_end_dict, self.mel_overlap_dict, self.hift_cache_dict, self.flow_cache_dict, self._llm_errors):
                d.pop(uuid_, None)

    def _emit(self, uuid_, producer, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, stream, speed, poll):
        """The token -> waveform schedule shared by tts (:173-238) and vc (:240-292): hop + overlap windows while streaming,
        one pass over everything otherwise."""
        kw = dict(prompt_token=flow_prompt_speech_token, prompt_feat=prompt_speech_feat, embedding=flow_embedding, uuid_=uuid_)
        toks = lambda k=None: torch.tensor(self.tts_speech_token_dict[uuid_][:k]).unsqueeze(dim=0)
        if stream:
            hop = self.token_min_hop_len
            while True:
                if poll:
                    time.sleep(poll)
                if len(self.tts_speech_token_dict[uuid_]) >= hop + self.token_overlap_len:
                    yield {"tts_speech": self.token2wav(token=toks(hop + self.token_overlap_len), finalize=False, **kw).cpu()}
                    with self.lock:
                        self.tts_speech_token_dict[uuid_] = self.tts_speech_token_dict[uuid_][hop:]
                    hop = min(self.token_max_hop_len, int(hop * self.stream_scale_factor))
                if self.llm_end_dict[uuid_] is True and len(self.tts_speech_token_dict[uuid_]) < hop + self.token_overlap_len:
                    break
            if producer is not None:
                producer.join()
                self._raise_llm_error(uuid_)
            yield {"tts_speech": self.token2wav(token=toks(), finalize=True, **kw).cpu()}
        else:
            if producer is not None:
                producer.join()
                self._raise_llm_error(uuid_)
            yield {"tts_speech": self.token2wav(token=toks(), finalize=True, speed=speed, **kw).cpu()}

    def _raise_llm_error(self, uuid_):
        err = self._llm_errors.pop(uuid_, None)
        if err is not None:
            raise err

    def tts(self, text, flow_embedding, llm_embedding=torch.zeros(0, 512), prompt_text=torch.zeros(1, 0, dtype=torch.int32),
            llm_prompt_speech_token=torch.zeros(1, 0, dtype=torch.int32), flow_prompt_speech_token=torch.zeros(1, 0, dtype=torch.int32),
            prompt_speech_feat=torch.zeros(1, 0, 80), stream=False, speed=1.0, **kwargs):
        this_uuid = str(uuid.uuid1())
        self._open(this_uuid, [], False)
        p = threading.Thread(target=self.llm_job, args=(text, prompt_text, llm_prompt_speech_token, llm_embedding, this_uuid))
        p.start()
        try:
            yield from self._emit(this_uuid, p, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, stream, speed, 0.1)
        finally:
            p.join()
            self._close(this_uuid)

    def vc(self, source_speech_token, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, stream=False, speed=1.0, **kwargs):
        this_uuid = str(uuid.uuid1())
        self._open(this_uuid, source_speech_token.flatten().tolist(), True)
        try:
            yield from self._emit(this_uuid, None, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, stream, speed, 0.0)
        finally:
            self._close(this_uuid)
