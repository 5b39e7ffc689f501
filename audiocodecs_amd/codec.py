"""Codec interface -- host-side mirror of the reference's `audiocodecs.Codec`
(/root/reference/audiocodecs/codec.py:33-214): same constructor, public methods, argument
meaning (relative `length`, [B,T] signals, [B,N,K] tokens) and error behaviour, so callers such as
downstream/test_sr.py:57,83 run unchanged.  The class skeleton (constructor, `_MODES`, method names, abstract obligations) IS the
drop-in boundary and necessarily reads like the reference's.  The token utilities at the end (`resample`, `logits`, `_sample_top_k`,
`_sample_top_p`) restate /root/reference/audiocodecs/codec.py:121-180 step for step -- host-side torch code off the kernel path, whose RNG
call order has to match for same-seed behaviour -- with device placement fixed; everything else (workspaces, graph mode, strict polling,
the native calls) is this repo's own.
"""

from __future__ import annotations

from abc import ABC, abstractmethod

import torch

from .resample import resample as _resample

__all__ = ["Codec"]


class Codec(torch.nn.Module, ABC):
    _MODES = ["encode", "decode", "reconstruct"]

    def __init__(self, sample_rate, orig_sample_rate, mode="reconstruct"):
        super().__init__()
        if mode not in self._MODES:
            raise ValueError(f"`mode` ({mode}) must be one of {self._MODES}")  # codec.py:38-39
        self.sample_rate = sample_rate
        self.orig_sample_rate = orig_sample_rate
        self.mode = mode
        self._logits = None
        # strict=True (keyword of every wrapper): after each public call, synchronise the stream and poll the handle for
        # failures only the device can see (a failed persistent LSTM launch, token ids out of range) so that THIS call raises,
        # not an unrelated later one (include/audiocodecs_amd.h: ac_poll_status).  Default off: no entry point synchronises.
        self.strict = False
        # graph=True (keyword of every wrapper): sig_to_toks / toks_to_sig replay ONE hipGraph per (call, shape) instead of launching their
        # 10 - 100 kernels one by one -- for the short calls of the reference's own measurement regime (batch 1, downstream/hparams/tasks/sr.yaml:28),
        # where launch gaps are a third of the call.  Default off.
        self.graph = False
        self._graphs = {}            # (call, shape, dtype, device) -> captured graph; at most GRAPH_CACHE, least recently used dropped
        self._graph_failed = set()

    # codec.py:45-55
    def forward(self, input, length=None):
        if self.mode == "encode":
            return self.sig_to_toks(input, length)
        if self.mode == "decode":
            return self.toks_to_sig(input, length)
        toks = self.sig_to_toks(input, length)
        return self.toks_to_sig(toks, length)

    def _in(self, sig):
        return _resample(sig, self.sample_rate, self.orig_sample_rate)

    def _out(self, sig):
        return _resample(sig, self.orig_sample_rate, self.sample_rate)

    _accepts_none_length = False  # subclasses that can skip the all-ones mask set this

    def _ones(self, x):
        # codec.py:64-65: length defaults to ones(B) -- the "no padding" case
        return None if self._accepts_none_length else torch.ones(len(x), device=x.device)

    def _handles(self):
        """Every live native handle of this wrapper (a wrapper with a second handle map -- Encodec's Vocos decoder -- adds it)."""
        return list(getattr(self, "_natives", {}).values())

    def _polled(self, out):
        """strict mode: surface device-side failures of the call that just ran (ac_poll_status synchronises the stream).  Every handle
        of the wrapper on the result's device is polled: the one that produced the result is among them."""
        first = out[0] if isinstance(out, (tuple, list)) and out else out      # (a wrapper method may return several tensors)
        if self.strict and isinstance(first, torch.Tensor) and first.is_cuda:
            from . import _native

            out_dev = first.device
            for nat in self._handles():
                if nat.device.index != out_dev.index:
                    continue
                with torch.cuda.device(out_dev):
                    stream = torch.cuda.current_stream().cuda_stream
                    _native.check(nat.lib.ac_poll_status(nat.h, stream), nat.h, "ac_poll_status")
        return out

    # ---- opt-in hipGraph replay of the two hot calls ---------------------------------------------------------------------------
    # The codecs with an LSTM (EnCodec, WavTokenizer) decline: their persistent cooperative launch cannot be replayed from a graph (a replay
    # does not get the XCD placement the exchange relies on), and the per-time-step kernels that serve under capture are
    # slower than the eager call -- measured, EnCodec 1 x 1 s: 2.05 ms replayed against 1.32 ms eager, 1 x 10 s: 12.5 against 3.8 -- and round
    # differently from the persistent kernel.  At batch 1 the eager call is kernel time anyway (1.30 ms of events in a 1.29 ms call): tiny
    # launches that walk a K = 4096 contraction on two workgroups, not launch gaps.  graph=True on those wrappers is accepted and has no effect.
    _graph_capable = True
    GRAPH_CACHE = 8               # graphs (each with a private workspace and static tensors) a codec keeps

    def _graph_ok(self, name) -> bool:
        """Whether call `name` ("sig_to_toks" / "toks_to_sig") may be replayed: per wrapper, or per call where a wrapper's calls differ."""
        return self._graph_capable

    def _graphed(self, name, fn, x, length):
        """fn(x, None) through a hipGraph captured once per (call, shape, dtype, device).  The first call of a key runs
        eagerly (creates the handle, sizes the workspace) and then captures a second run into static input / output tensors; later calls
        copy their input in, replay, and return a COPY of the static output (a caller may hold results across calls).  Every entry point of
        the library is capturable (no allocation, no synchronisation inside: include/audiocodecs_amd.h).  Results are bit-identical to the
        eager call's (tests/test_graph_mode_gpu.py)."""
        # (a caller-provided `length` is checked on the host by some wrappers -- encodec.py:84-89's mask size -- which a capture cannot do: eager)
        if not (self.graph and self._graph_ok(name) and isinstance(x, torch.Tensor) and x.is_cuda and x.shape[0] > 0 and length is None):
            return fn(x, length)
        key = (name, tuple(x.shape), x.dtype, x.device.index)
        ent = self._graphs.get(key)
        if ent is not None:
            self._graphs[key] = self._graphs.pop(key)             # most recently used last
        elif key in self._graph_failed:
            return fn(x, length)                                  # this shape's capture failed once: eager from then on
        if ent is None:
            out = fn(x, length)                                   # eager: handle, workspace, LDS opt-ins
            if torch.cuda.is_current_stream_capturing():
                return out                                        # (a caller's own capture: stay out of its way)
            # Graph mode is for FIXED shapes (a serving loop at one batch and length): every new (call, shape) costs an eager call plus a
            # capture and then pins a private workspace and static input / output tensors.  The cache therefore holds the GRAPH_CACHE most
            # recently used graphs and drops the oldest (its workspace with it); variable-length callers should bucket their lengths or
            # leave graph mode off.
            while len(self._graphs) >= self.GRAPH_CACHE:
                self._graphs.pop(next(iter(self._graphs)))
            sx = x.clone()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            # The graph bakes in the address of the workspace it was captured with, and the wrapper's own workspace tensor is REPLACED when a
            # later call needs a larger one: every graph gets a workspace of its own (allocated inside the capture, from the graph's private
            # pool, and kept alive with the graph), the wrapper's is put back afterwards.
            nats = self._handles()
            kept = [n.ws for n in nats]
            for n in nats:
                n.ws = None
            try:
                with torch.cuda.stream(side):
                    with torch.cuda.graph(g, stream=side):
                        so = fn(sx, None)
                own = [n.ws for n in nats]
            except Exception:                                     # a failed capture (out of memory for the private workspace, ...) must not
                self._graph_failed.add(key)                       # fail the call: the eager result is already in hand
                for n, w in zip(nats, kept):
                    n.ws = w
                torch.cuda.current_stream(x.device).wait_stream(side)
                return out
            for n, w in zip(nats, kept):
                n.ws = w
            torch.cuda.current_stream(x.device).wait_stream(side)
            self._graphs[key] = (g, sx, so, own)
            return out
        g, sx, so, _ = ent
        sx.copy_(x)
        g.replay()
        return so.clone()

    def sig_to_toks(self, sig, length=None):  # codec.py:57-66
        sig = self._in(sig)
        if self.graph:
            return self._polled(self._graphed("sig_to_toks", lambda s_, l_: self._sig_to_toks(s_, self._ones(s_) if l_ is None else l_), sig, length))
        return self._polled(self._sig_to_toks(sig, self._ones(sig) if length is None else length))

    def sig_to_feats(self, sig, length=None):  # codec.py:68-77
        sig = self._in(sig)
        return self._polled(self._sig_to_feats(sig, self._ones(sig) if length is None else length))

    def sig_to_qfeats(self, sig, length=None):  # codec.py:79-88
        sig = self._in(sig)
        return self._polled(self._sig_to_qfeats(sig, self._ones(sig) if length is None else length))

    def toks_to_sig(self, toks, length=None):  # codec.py:90-100
        if self.graph:
            sig = self._polled(self._graphed("toks_to_sig", lambda t_, l_: self._toks_to_sig(t_, self._ones(t_) if l_ is None else l_), toks, length))
        else:
            sig = self._polled(self._toks_to_sig(toks, self._ones(toks) if length is None else length))
        return self._out(sig)

    def toks_to_qfeats(self, toks, length=None):  # codec.py:102-107
        return self._polled(self._toks_to_qfeats(toks, self._ones(toks) if length is None else length))

    def feats_to_sig(self, feats, length=None):  # codec.py:109-119
        sig = self._polled(self._feats_to_sig(feats, self._ones(feats) if length is None else length))
        return self._out(sig)

    def knn_vc(self, toks, spk_sigs, topk=4):
        """Single-codebook voice conversion by k-NN feature matching (downstream/test_vc.py:116-128): every quantised feature of `toks`
        [B, N, 1] is replaced by the mean of its `topk` nearest continuous features (cosine similarity) of the target speaker's signals
        `spk_sigs` -- a list of [T] or [1, T] signals at `self.sample_rate` -- and the result is decoded: [B, T'].  Built from the
        public methods and `knn_match` (knn.py) only.  Multi-codebook codecs convert by token splicing (test_vc.py:102-114), which needs
        no kernel: a `toks` with K != 1 is a ValueError."""
        from .knn import knn_match

        if toks.dim() != 3 or toks.shape[-1] != 1:
            raise ValueError(f"knn_vc is the single-codebook conversion: `toks` must be [B, N, 1] (got {tuple(toks.shape)})")
        if type(self)._feats_to_sig is Codec._feats_to_sig:
            raise NotImplementedError     # (before any work: this wrapper cannot decode features)
        if not spk_sigs:
            raise ValueError("`spk_sigs` is empty: there is nothing to match")
        matching_set = torch.cat([self.sig_to_feats(s[None] if s.dim() == 1 else s).flatten(end_dim=-2) for s in spk_sigs])
        return self.feats_to_sig(knn_match(self.toks_to_qfeats(toks), matching_set, topk))

    def probe(self, sig, probe, length=None):
        """`sig_to_toks`, then a `TokenProbe` (probe.py) over the tokens -> its `ProbeOutput`.  `length` is relative, as everywhere in this
        class; the probe gets round(length * N) frames per clip (`probe.relative_to_frames`), computed on the device.  Built from the
        public methods only."""
        from .probe import relative_to_frames

        toks = self.sig_to_toks(sig, length)
        if length is None:
            return probe.forward(toks)
        if not torch.is_tensor(length):
            length = torch.as_tensor(length, dtype=torch.float32)
        return probe.forward(toks, relative_to_frames(length.to(toks.device), toks.shape[1]))

    def _resynthesize(self, sig, length):
        """`sig_to_toks`, `toks_to_sig` and the length adjustment of downstream/test_sr.py:89-100 (the decode is replicate-padded or narrowed
        to the input's length): (toks [B, N, K], hyp [B, T])."""
        if not torch.is_tensor(sig) or sig.dim() != 2:
            raise ValueError("`sig` must be a [B, T] tensor")
        toks = self.sig_to_toks(sig, length)
        hyp = self.toks_to_sig(toks, length)
        T = sig.shape[-1]
        if T > hyp.shape[-1]:
            hyp = torch.nn.functional.pad(hyp, [0, T - hyp.shape[-1]], mode="replicate")
        elif T < hyp.shape[-1]:
            hyp = hyp.narrow(-1, 0, T)
        return toks, hyp

    def resynthesis_distances(self, sig, length=None):
        """The STFT and mel spectral distances of this codec's resynthesis of `sig` [B, T] (at `self.sample_rate`) against `sig` itself:
        `sig_to_toks`, `toks_to_sig`, the length adjustment of downstream/test_sr.py:89-100 (the decode is replicate-padded or narrowed to
        the input's length) and `spectral_distances` (metrics.py) -- (stft [B], mel [B]).  Built from the public methods only."""
        from .metrics import spectral_distances

        hyp = self._resynthesize(sig, length)[1]      # (the tokens go here, before the metric allocates)
        return spectral_distances(hyp, sig.to(hyp.dtype), self.sample_rate)

    def resynthesis_stoi(self, sig, length=None):
        """The STOI of this codec's resynthesis of `sig` [B, T] (at `self.sample_rate`) against `sig` itself: `sig_to_toks`, `toks_to_sig`,
        the length adjustment of downstream/test_sr.py:89-100 and `stoi` (metrics.py) with `sig` as the reference -- [B].  Built from
        the public methods only."""
        from .metrics import stoi

        hyp = self._resynthesize(sig, length)[1]      # (the tokens go here, before the metric allocates)
        return stoi(hyp, sig.to(hyp.dtype), self.sample_rate)

    def resynthesis_dnsmos(self, sig, weights, length=None):
        """The DNSMOS (P.808) of this codec's resynthesis of `sig` [B, T] (at `self.sample_rate`): `sig_to_toks`, `toks_to_sig`, the length
        adjustment of downstream/test_sr.py:89-100 and `dnsmos` (dnsmos.py) of the decode -- [B].  `weights` is a `DnsmosWeights` or the path of
        the P.808 weights.  Built from the public methods only."""
        from .dnsmos import dnsmos

        hyp = self._resynthesize(sig, length)[1]      # (the tokens go here, before the metric allocates)
        return dnsmos(hyp, self.sample_rate, weights)

    def resynthesis_spk_sim(self, sig, encoder, length=None):
        """The WavLM x-vector speaker similarity of this codec's resynthesis of `sig` [B, T] (at `self.sample_rate`) against `sig` itself:
        `sig_to_toks`, `toks_to_sig`, the length adjustment of downstream/test_sr.py:89-100 and `speaker_similarity` (spksim.py) with a
        `SpeakerEncoder` -- [B].  `length` also masks both signals in the encoder.  Built from the public methods only."""
        from .spksim import speaker_similarity

        hyp = self._resynthesize(sig, length)[1]      # (the tokens go here, before the metric allocates)
        return speaker_similarity(hyp, sig.to(hyp.dtype), self.sample_rate, encoder, length)

    def resynthesis_report(self, sig, length=None, dnsmos_weights=None, codebook_util=None):
        """The recipe's numbers for a batch from ONE encode and ONE decode (downstream/test_sr.py:83-112): `sig_to_toks`, `toks_to_sig`, the
        length adjustment of test_sr.py:89-100 once, then `spectral_distances`, `stoi` and, with `dnsmos_weights` (a `DnsmosWeights` or the
        path of the P.808 weights), `dnsmos` of the decode; a `CodebookUtil` (tokstats.py) passed as `codebook_util` gets the tokens
        appended with `length`.  Returns {"toks" [B, N, K], "stft" [B], "mel" [B], "stoi" [B]} and "dnsmos" [B] when weights were given:
        what `resynthesis_distances`, `resynthesis_stoi` and `resynthesis_dnsmos` return, which encode and decode once each.  Built from
        the public methods only."""
        from .metrics import spectral_distances, stoi

        toks, hyp = self._resynthesize(sig, length)
        ref = sig.to(hyp.dtype)
        report = {"toks": toks}
        report["stft"], report["mel"] = spectral_distances(hyp, ref, self.sample_rate)
        report["stoi"] = stoi(hyp, ref, self.sample_rate)
        if dnsmos_weights is not None:
            from .dnsmos import dnsmos

            report["dnsmos"] = dnsmos(hyp, self.sample_rate, dnsmos_weights)
        if codebook_util is not None:
            codebook_util.append(toks, length)
        return report

    # ---- token-resampling utilities: a step-for-step restatement of /root/reference/audiocodecs/codec.py:121-180 (same RNG call order;
    #      no caller in the reference tree) --------
    #      With a `seed` the same resampling runs as one launch of the library (sampling.py): the draws come from
    #      the repository's counter-based PRNG at `(seed, offset)`, not from torch's generator.
    def resample(self, toks, p=0.2, temp=1.0, top_k=None, top_p=None, seed=None, offset=0):
        if seed is not None:
            if p <= 0.0:
                return toks
            from .sampling import resample_tokens

            return resample_tokens(toks, self.logits(), p, temp=temp, top_k=top_k, top_p=top_p, seed=seed, offset=offset)
        if p <= 0.0:
            return toks
        out = toks.clone()
        K = toks.shape[-1]
        flat = toks.flatten(end_dim=-2).T  # [K, BN]
        logits = self.logits()  # [K, C, C]
        vocab = logits.shape[-1]
        sel = logits.gather(1, flat[..., None].expand(-1, -1, vocab)).flatten(end_dim=-2)  # [K*BN, C]
        probs = (sel / temp).softmax(dim=-1)
        if top_k is None and top_p is None:
            samples = probs.multinomial(num_samples=1)
        elif top_k is not None and top_p is None:
            samples = self._sample_top_k(probs, top_k)
        elif top_k is None and top_p is not None:
            samples = self._sample_top_p(probs, top_p)
        else:
            raise NotImplementedError
        samples = samples.reshape(K, -1).T.reshape_as(out)
        mask = torch.rand(out.shape, device=out.device) < p
        out[mask] = samples[mask]
        return out

    @torch.no_grad()
    def logits(self):
        if self._logits is None:
            embs = self.embs()  # [K, C, H]
            logits = -torch.cdist(embs, embs)
            eye = torch.eye(logits.shape[-1], device=logits.device).bool().expand(len(logits), -1, -1)
            logits[eye] = -float("inf")
            self._logits = logits
        return self._logits.clone()

    def _sample_top_k(self, probs, k):
        probs, idx = probs.topk(k, dim=-1)
        probs = probs / probs.sum(dim=-1, keepdim=True)
        return idx.gather(-1, probs.multinomial(num_samples=1))[:, 0]

    def _sample_top_p(self, probs, p):
        probs, idx = probs.sort(dim=-1, descending=True)
        csum = probs.cumsum(dim=-1)
        probs = probs.masked_fill(csum - probs > p, 0.0)
        probs = probs / probs.sum(dim=-1, keepdim=True)
        return idx.gather(-1, torch.multinomial(probs, num_samples=1))[:, 0]

    # ---- subclass obligations (codec.py:182-214) ------------------------------------------------
    @abstractmethod
    def embs(self):
        raise NotImplementedError

    @abstractmethod
    def _sig_to_toks(self, sig, length):
        raise NotImplementedError

    @abstractmethod
    def _sig_to_feats(self, sig, length):
        raise NotImplementedError

    @abstractmethod
    def _sig_to_qfeats(self, sig, length):
        raise NotImplementedError

    @abstractmethod
    def _toks_to_sig(self, toks, length):
        raise NotImplementedError

    def _toks_to_qfeats(self, toks, length):
        raise NotImplementedError

    def _feats_to_sig(self, feats, length):
        raise NotImplementedError
