"""Step-wise incremental decoding driver: the model side of the reference's generation loop
(generator/sequence_generator.py:258-306 -- encoder once, then one decoder call per step with an `incremental_state`,
beams reordered in between) with the launch-bound step captured into hipGraphs.

One decoding step of OFA-base is ~130 small kernels; launched eagerly from Python it takes 2.65 ms whether 32 or 160 rows
are decoded (host-bound).  `StepDecoder` keeps every buffer a step touches at a fixed address -- target tokens, encoder
output, the KV caches at their final capacity -- and records ONE hipGraph PER STEP LENGTH (the prefix length and the cache
length are kernel arguments, so each length is its own graph; a sequence of T steps replays T graphs).  Graphs are keyed by
(rows, source length, step) -- plus the `variant` a caller passes to `step` when it records different work at one step -- and reused
by every later batch of the same shape.  `greedy` below is the minimal loop used
by tests and benchmarks.  With `features_only` a step returns the last position's features [rows, D] instead of logits (the
output projection is not run): what `TrieBeamGenerator` consumes.

`SequenceGenerator` is the reference's beam search (generator/sequence_generator.py:66-627 with utils/search.py BeamSearch)
on top of `StepDecoder`: the policy of a step -- normaliser, masks, n-gram bans, top 2K, finalisation, active selection,
history gather -- is two HIP launches (csrc/beam_search.hip) recorded with the decoder and the self-attention cache reorder
into the step's graph, so a step has no host synchronisation.  Differences from the reference ("Generation
(beam search)"):
the row count stays fixed (finished sentences are masked, not removed; rows are independent, so results are the same),
the returned tensors are on the CPU, and `attention` is empty (the decoder returns no alignment).
A sample whose `prefix_tokens` has columns (a target that opens with fixed text) is decoded one token per step like any other:
while a sentence's prefix lasts, its rows are forced onto the prefix token by three launches (`_prefix_step_kernels`).

`TrieBeamGenerator` is the same search restricted, at every step, to the next layer of a closed set's answer trie (the reference's
`constraint_trie`, generator/sequence_generator.py:729-741): the row pass computes one dot product per child edge of the row's trie
node instead of reading a [rows, V] projection (csrc/trie_beam.hip), the sentence pass is unchanged, and a third small launch
advances every row's node.

`SequenceGenerator(search_strategy=Sampling(...))` samples instead (utils/search.py:596-715): a sentence's K rows are K independent
samples, drawn by csrc/sample.hip from uniform numbers held in `st["uniforms"]` -- supplied by the caller (`generate(uniforms=U)`) or
filled once per generate, outside the step graphs, from a seeded torch.Generator.

`SequenceGenerator(search_strategy=DiverseBeamSearch(...) | DiverseSiblingsSearch(...))` decodes diversely (utils/search.py:532-593,
718-787): the row pass, the decoder step and the cache reorder are the plain ones, and the sentence pass is csrc/diverse_beam.hip's,
which works on the candidates the row pass already lists.

`AutoRegressiveSpeechGenerator` is the reference's generator of fbank frames (generator/speech_generator.py:84-200) on
`SpeechStepDecoder`, a `StepDecoder` that feeds the decoder one embedded frame per step: the step's policy -- fbank head, sigmoid,
finish rule, next padding flag, finished count, prenet of the new frame -- is one HIP launch (csrc/speech_step.hip) recorded with the
decoder into the step's graph.
"""
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch

from . import kernels as K
from .preprocessor import ModalityType, Slot


class StepDecoder:
    def __init__(self, model, max_len: int, use_graph: bool = True, warmup_sequences: int = 1, features_only: bool = False):
        self.model, self.max_len, self.use_graph = model, int(max_len), use_graph
        self.warmup_sequences = warmup_sequences
        self.features_only = bool(features_only)          # a step returns [rows, D] features; the output projection is skipped
        self._shape = None
        self._graphs: Dict[Any, tuple] = {}              # step, or (step, variant)
        self._pool = None
        self._seq = 0
        self._ws: Dict[tuple, torch.Tensor] = {}          # scratch buffers allocated inside this decoder's captures (see step)
        self._ws_keep: List[torch.Tensor] = []

    # ------------------------------------------------------------------ sequence state
    def begin(self, src_slots: List[Slot], beam_order: Optional[torch.Tensor] = None):
        """Encode the sources (eagerly), optionally expand to beams (`beam_order`: row index per output row), and point the
        static buffers at the new batch."""
        m = self.model
        m.eval()                                          # decoding is an inference-mode activity: the model STAYS in eval mode (call
        #                                                   model.train() before the next train step, as with the reference's generator)
        for mod in m.decoder.modules():                   # packed decode projections follow the current parameters
            if getattr(mod, "_decode_pack_cache", None) is not None:
                mod._decode_pack()
        with torch.no_grad():
            enc = m.encoder(src_slots)
            if beam_order is not None:
                enc = m.encoder.reorder_encoder_out(enc, beam_order)
        out = enc["encoder_out"][0]
        # captured step graphs bake in parameter ADDRESSES: a TrainStep built afterwards (its arenas re-point p.data) or a
        # model.to(...) must drop them, so the storage of one parameter is part of the cache key
        fingerprint = next(m.decoder.parameters()).data_ptr()
        shape = (out.shape[1], out.shape[0], out.dtype, fingerprint)
        if shape != self._shape:                          # another batch shape: new buffers, new graphs
            self._shape, self._graphs, self._pool, self._seq = shape, {}, None, 0
            self._ws, self._ws_keep = {}, []
            self.enc = {k: [t.clone() if torch.is_tensor(t) else t for t in v] if isinstance(v, list) else v for k, v in enc.items()}
            self.tokens = torch.zeros(shape[0], self.max_len, dtype=torch.long, device=out.device)
            self.inc = {"__capacity__": self.max_len, "__static__": True}
        else:
            with torch.no_grad():
                for k, v in enc.items():
                    if isinstance(v, list):
                        for dst, srct in zip(self.enc[k], v):
                            if torch.is_tensor(dst):
                                dst.copy_(srct)
            for mod in m.decoder.modules():
                if hasattr(mod, "reset_incremental_state"):
                    mod.reset_incremental_state(self.inc)
            self._seq += 1
        self.t = 0
        return self

    def step(self, next_tokens: Optional[torch.Tensor], post=None, variant=None) -> torch.Tensor:
        """Append one token per row and return the logits of that position: [rows, V] ([rows, D] features with `features_only`).
        next_tokens None: column t of `tokens` was already written on the device (beam search).  post(logits, t): device work
        recorded into the same step graph after the decoder (the beam-search kernels and the cache reorder).  variant (hashable):
        names what `post` records when that differs between sequences at one step -- a graph is replayed only for its own variant."""
        t = self.t
        key = t if variant is None else (t, variant)
        if t >= self.max_len:
            raise ValueError(f"StepDecoder: max_len={self.max_len} exceeded")
        if next_tokens is not None:
            self.tokens[:, t].copy_(next_tokens.reshape(-1))
        graphed = self.use_graph and self._seq >= self.warmup_sequences
        if graphed and key in self._graphs:
            g, logits = self._graphs[key]
            self._set_lengths(t + 1)
            g.replay()
        elif graphed:
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            # the decoder's captures see only their own scratch (kernels.capture_workspaces), kept alive for as long as its graphs
            with K.capture_workspaces(self._ws) as added, torch.no_grad(), \
                    torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
                logits = self._run(t)
                if post is not None:
                    post(logits, t)
            self._ws_keep.extend(added.values())
            if self._pool is None:
                self._pool = g.pool()
            self._graphs[key] = (g, logits)
            g.replay()                                    # capture only records: run the step once
        else:
            with torch.no_grad():
                logits = self._run(t)
                if post is not None:
                    post(logits, t)
        self.t = t + 1
        return logits

    def _run(self, t):
        kw = {"features_only": True} if self.features_only else {}
        out, _ = self.model.decoder([Slot(ModalityType.TEXT, False, self.tokens[:, :t + 1])], encoder_out=self.enc,
                                    incremental_state=self.inc, **kw)
        return out[:, -1]

    def _set_lengths(self, n):
        """The host-side cache lengths (only read when a step is recorded or run eagerly) follow the replayed steps."""
        for c in self.inc.values():
            if isinstance(c, dict) and "len" in c and not c.get("static"):
                c["len"] = n
        return n

    def reorder(self, new_order: torch.Tensor, caches_only: bool = False):
        """Beam reorder between steps: caches, encoder output and the token prefix follow `new_order` (in place).
        caches_only: the self-attention caches alone -- beams that move within their sentence (beam search) share the encoder
        output and the cross-attention cache, and the token history is gathered by the beam kernels.  `new_order` is read on
        the device only (no host synchronisation), so the call can be recorded into a step graph with the index at a fixed
        address."""
        m = self.model
        if new_order.numel() != self._shape[0]:
            raise ValueError("StepDecoder.reorder keeps the row count (the buffers of the captured steps are fixed): "
                             f"got {new_order.numel()} indices for {self._shape[0]} rows")
        m.decoder.reorder_incremental_state_scripting(self.inc, new_order)
        if caches_only:
            return
        enc = m.encoder.reorder_encoder_out(self.enc, new_order)
        for k, v in enc.items():
            if isinstance(v, list):
                for dst, srct in zip(self.enc[k], v):
                    if torch.is_tensor(dst):
                        dst.copy_(srct)
        self.tokens.copy_(self.tokens.index_select(0, new_order))

    # ------------------------------------------------------------------ minimal loop
    def greedy(self, src_slots: List[Slot], bos: int, steps: int, beam_order: Optional[torch.Tensor] = None):
        """Forced-length greedy decoding: returns tokens [rows, steps + 1] (bos first) and the per-step logits."""
        self.begin(src_slots, beam_order)
        rows = self._shape[0]
        nxt = torch.full((rows,), bos, dtype=torch.long, device=self.tokens.device)
        logits_all = []
        for _ in range(steps):
            logits = self.step(nxt)
            logits_all.append(logits.float().clone())
            nxt = logits.argmax(-1)
        toks = torch.cat([self.tokens[:, :steps], nxt.view(-1, 1)], 1)
        return toks, torch.stack(logits_all)


# ---------------------------------------------------------------------------------------------------------------- beam search
@dataclass
class SequenceGeneratorOutput:
    """One finalised hypothesis (generator/sequence_generator.py:25-40): tokens 1..n ending in EOS, its (length-normalised)
    score, the positional scores, and the decoded forms a task fills in."""
    tokens: torch.LongTensor
    score: torch.FloatTensor
    attention: torch.FloatTensor
    positional_scores: torch.FloatTensor
    text: Optional[str] = None
    image: Any = None
    box: Optional[torch.Tensor] = None


class Sampling:
    """The reference's sampling search strategy (utils/search.py:596-603) as a plain options holder: what
    `SequenceGenerator(search_strategy=...)` reads.  sampling_topp > 0 (nucleus) wins over sampling_topk > 0; neither: the whole
    vocabulary.  The step itself is csrc/sample.hip."""

    def __init__(self, tgt_dict, sampling_topk=-1, sampling_topp=-1.0):
        self.pad, self.unk, self.eos, self.vocab_size = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos(), len(tgt_dict)
        self.sampling_topk, self.sampling_topp = int(sampling_topk), float(sampling_topp)
        if self.sampling_topp > 1.0:
            raise ValueError(f"Sampling: sampling_topp={sampling_topp} is above 1")


class DiverseBeamSearch:
    """The reference's diverse beam search (utils/search.py:532-547; Hamming diversity between `num_groups` groups of beams) as a
    plain options holder.  The step is csrc/diverse_beam.hip's ofa_diverse_group_select, which needs a strength >= 0."""

    def __init__(self, tgt_dict, num_groups, diversity_strength):
        self.pad, self.unk, self.eos, self.vocab_size = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos(), len(tgt_dict)
        self.num_groups, self.diversity_strength = int(num_groups), float(diversity_strength)
        if self.num_groups < 1:
            raise ValueError(f"DiverseBeamSearch: num_groups={num_groups} is below 1")
        if not (0.0 <= self.diversity_strength < math.inf):
            raise ValueError(f"DiverseBeamSearch: diversity_strength={diversity_strength} must be finite and >= 0 (a negative "
                             "strength rewards repeated tokens; the step then needs more than each row's top 2K candidates)")


class DiverseSiblingsSearch:
    """The reference's diverse-siblings search (utils/search.py:718-736) as a plain options holder; rate 0 is plain beam search.
    The step is csrc/diverse_beam.hip's ofa_diverse_sibling_select."""

    def __init__(self, tgt_dict, diversity_rate):
        self.pad, self.unk, self.eos, self.vocab_size = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.eos(), len(tgt_dict)
        self.diversity_rate = float(diversity_rate)
        if not math.isfinite(self.diversity_rate):
            raise ValueError(f"DiverseSiblingsSearch: diversity_rate={diversity_rate} is not finite")


class SequenceGenerator:
    """Beam search with the reference's constructor and defaults (generator/sequence_generator.py:66-159), or sampling with
    `search_strategy=Sampling(...)` (`seed`: of the uniform numbers `generate` draws when it is given none; None: taken from
    torch's global generator), or diverse decoding with `search_strategy=DiverseBeamSearch(...)` / `DiverseSiblingsSearch(...)`.
    Unsupported options of the reference raise NotImplementedError: other search strategies, an LM, a constraint trie,
    match_source_len, lexical constraints, a prefix that holds <eos>, and any prefix under sampling or diverse decoding."""

    MAX_BEAM = 16

    def __init__(self, tgt_dict, beam_size: int = 1, return_n_best: int = -1, max_len_a: int = 0, max_len_b: int = 200,
                 max_len: int = 256, min_len: int = 1, normalize_scores: bool = True, len_penalty: float = 1.0,
                 unk_penalty: float = 0.0, temperature: float = 1.0, match_source_len: bool = False,
                 no_repeat_ngram_size: int = 0, search_strategy=None, lm_model=None, lm_weight: float = 1.0,
                 constraint_trie=None, constraint_range: Optional[str] = None, use_graph: bool = True, seed: Optional[int] = None,
                 **unused_kwargs):
        if search_strategy is not None and not isinstance(search_strategy, (Sampling, DiverseBeamSearch, DiverseSiblingsSearch)):
            raise NotImplementedError("SequenceGenerator: only plain beam search, sampling and diverse decoding are implemented "
                                      "(search_strategy must be None, a Sampling, a DiverseBeamSearch or a DiverseSiblingsSearch; "
                                      "constrained search is not)")
        self.sampling: Optional[Sampling] = search_strategy if isinstance(search_strategy, Sampling) else None
        self.diverse = search_strategy if isinstance(search_strategy, (DiverseBeamSearch, DiverseSiblingsSearch)) else None
        self.seed, self._rng = seed, None
        if lm_model is not None:
            raise NotImplementedError("SequenceGenerator: LM fusion (lm_model) is not implemented")
        if constraint_trie is not None:
            raise NotImplementedError("SequenceGenerator: constraint_trie (a host-side trie walk per step) is not implemented; "
                                      "constraint_range is")
        if match_source_len:
            raise NotImplementedError("SequenceGenerator: match_source_len is not implemented")
        if not temperature > 0:
            raise ValueError("--temperature must be greater than 0")
        self.pad, self.unk, self.bos, self.eos = tgt_dict.pad(), tgt_dict.unk(), tgt_dict.bos(), tgt_dict.eos()
        self.vocab_size = len(tgt_dict)
        self.beam_size = min(beam_size, self.vocab_size - 1)
        if self.beam_size > self.MAX_BEAM:
            raise NotImplementedError(f"SequenceGenerator: beam_size {beam_size} > {self.MAX_BEAM} (csrc/beam_search.hip)")
        if return_n_best == -1:
            return_n_best = self.beam_size
        self.return_n_best = min(self.beam_size, return_n_best)
        if isinstance(self.diverse, DiverseBeamSearch) and self.beam_size % self.diverse.num_groups != 0:
            raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
        if isinstance(self.diverse, DiverseSiblingsSearch) and self.vocab_size <= 2 * self.beam_size:
            raise ValueError(f"DiverseSiblingsSearch: every beam lists its own top 2 * beam = {2 * self.beam_size} tokens, the "
                             f"dictionary has {self.vocab_size}")
        self.max_len_a, self.max_len_b, self.max_len, self.min_len = max_len_a, max_len_b, max_len, min_len
        self.normalize_scores, self.len_penalty, self.unk_penalty = normalize_scores, len_penalty, unk_penalty
        self.temperature, self.no_repeat_ngram_size = temperature, no_repeat_ngram_size
        self.constraint_start, self.constraint_end = None, None
        if constraint_range is not None:
            self.constraint_start, self.constraint_end = (int(v) for v in str(constraint_range).strip("()[] ").split(","))
        self.use_graph = use_graph
        self._dec: Optional[StepDecoder] = None
        self._state: Optional[Dict[str, torch.Tensor]] = None
        self.steps_run = 0                                # decoding steps launched by the last generate()

    def effective_max_len(self, sample) -> int:
        """The output length limit the reference applies.  Its source-length rule (min(max_len, max_len_a * src_len + max_len_b),
        sequence_generator.py:185-217) never fires: the text-slot filter at :180-182 compares `x.modality == ModalityType` -- the
        enum CLASS -- which is always false, so src_len is None and the limit is max_len.  Reproduced as is."""
        return self.max_len

    def check_sample(self, sample, **kwargs) -> bool:
        """Refuse what is not implemented; returns whether the step-0 n-gram bans apply.  A collated batch always carries
        `prefix_tokens`; for a plain target it is [bsz, 0], which the reference treats as no prefix (`step < prefix_tokens.size(1)`
        never holds).  One trace of an empty prefix remains: the n-gram blocker skips rows whose prefix is not shorter than
        step + n - 1 (:319-327), so with n = 1 nothing is banned at step 0.  A prefix with columns is accepted in the form the
        collator builds (`_prefix_of`); checked once per generate."""
        if kwargs.get("constraints") is not None:
            raise NotImplementedError("SequenceGenerator: lexical constraints are not implemented")
        prefix = sample.get("prefix_tokens")
        self._prefix_of(sample)
        return not (prefix is not None and self.no_repeat_ngram_size == 1)

    def _prefix_of(self, sample):
        """(prefix [bsz, W] int64, plen [bsz]) of a sample whose prefix has columns, else None.  The collator strips BOS and EOS
        and pads on the right up to the longest prefix of the batch; what it cannot produce is refused: <eos> inside (the
        reference then copies the first beam over all beams, :509-522), <bos>, ids outside the dictionary, <pad> in front of a
        token, and a width that no row fills."""
        prefix = sample.get("prefix_tokens")
        if prefix is None or prefix.dim() != 2 or prefix.size(1) == 0:
            return None
        if self.sampling is not None:
            raise NotImplementedError("SequenceGenerator: prefix_tokens under sampling are not implemented (got a prefix of "
                                      f"{prefix.size(1)} columns)")
        if self.diverse is not None:
            raise NotImplementedError("SequenceGenerator: prefix_tokens under a diverse search strategy are not implemented (got a "
                                      f"prefix of {prefix.size(1)} columns)")
        prefix = prefix.long()
        keep = prefix.ne(self.pad)
        plen = keep.sum(1)
        W = prefix.size(1)
        ragged = (keep != (torch.arange(W, device=prefix.device).unsqueeze(0) < plen.unsqueeze(1))).any()
        facts = torch.stack([prefix.eq(self.eos).any(), prefix.eq(self.bos).any(), (prefix.lt(0) | prefix.ge(self.vocab_size)).any(),
                             ragged, plen.max().lt(W)]).tolist()                # one host read
        for bad, what in zip(facts, ("<eos>", "<bos>", "a token id outside the dictionary", "<pad> in front of a token",
                                     "only <pad> in its last column")):
            if bad:
                raise NotImplementedError(f"SequenceGenerator: prefix_tokens with {what} are not implemented (the collator's "
                                          "prefixes are right-padded and hold neither <bos> nor <eos>)")
        return prefix, plen

    # ------------------------------------------------------------------ device state
    def _buffers(self, rows, bsz, V, max_len, device):
        key = (rows, V, max_len, device)
        if self._state is None or self._state["key"] != key:
            K_ = self.beam_size
            i32 = dict(dtype=torch.int32, device=device)
            self._state = {
                "key": key,
                "ws": torch.empty((K.beam_ws_bytes(rows, V, K_) + 3) // 4, dtype=torch.float32, device=device),
                "scores": torch.zeros(rows, max_len + 1, dtype=torch.float32, device=device),
                "ignore": torch.zeros(bsz, K_, **i32), "done": torch.zeros(bsz, **i32), "nfin": torch.zeros(1, **i32),
                "reorder": torch.arange(rows, dtype=torch.long, device=device),
                "fin_tok": torch.zeros(bsz, K_, max_len + 1, dtype=torch.long, device=device),
                "fin_pos": torch.zeros(bsz, K_, max_len + 1, dtype=torch.float32, device=device),
                "fin_score": torch.zeros(bsz, K_, dtype=torch.float32, device=device),
                "fin_len": torch.zeros(bsz, K_, **i32), "fin_cnt": torch.zeros(bsz, **i32),
                "host": torch.zeros(2, dtype=torch.int32, pin_memory=True),
                # a forced target prefix, at fixed addresses for the step graphs: tokens (pad beyond a sentence's prefix), lengths,
                # and the prefix steps' scaled logit of every row's prefix token
                "prefix": torch.full((bsz, max_len + 1), self.pad, dtype=torch.long, device=device),
                "plen": torch.zeros(bsz, **i32), "glogit": torch.zeros(rows, dtype=torch.float32, device=device),
            }
            if self.sampling is not None:
                # the draws of a step and the uniform numbers of every step (step t reads row t), at fixed addresses
                self._state["sample_ws"] = torch.zeros((K.sample_ws_bytes(rows, V, K_) + 3) // 4, dtype=torch.float32, device=device)
                self._state["uniforms"] = torch.zeros(max_len + 1, rows, dtype=torch.float32, device=device)
        st = self._state
        for name in ("scores", "ignore", "done", "nfin", "fin_cnt"):
            st[name].zero_()
        st["reorder"].copy_(torch.arange(rows, dtype=torch.long, device=device))
        return st

    # ------------------------------------------------------------------ what TrieBeamGenerator overrides
    def _setup(self, model, max_len, device):
        """Before the loop: (steps after the first, i.e. the longest hypothesis without its EOS; the vocabulary width of the
        state; whatever `_row_pass` and `_advance` need)."""
        return max_len, self.vocab_size, None

    def _decoder(self, model, capacity):
        if self._dec is None or self._dec.model is not model:
            self._dec = StepDecoder(model, capacity, use_graph=self.use_graph)
        return self._dec

    def _check_output(self, logits):
        if logits.shape[1] > self.vocab_size:
            raise ValueError(f"decoder output width {logits.shape[1]} > dictionary size {self.vocab_size}")

    def _policy(self, dec, st, max_len, ngram):
        """The row passes' keywords (kernels._gen_policy)."""
        return dict(tokens=dec.tokens, done=st["done"], temperature=self.temperature, min_len=self.min_len, max_len=max_len,
                    constraint_range=None if self.constraint_start is None else (self.constraint_start, self.constraint_end),
                    pad=self.pad, unk=self.unk, eos=self.eos, unk_penalty=self.unk_penalty, ngram=ngram)

    def _select(self):
        """The sentence passes' keywords; the plain and prefix beam passes take the unk penalty as well."""
        kw = dict(eos=self.eos, normalize=self.normalize_scores, len_penalty=self.len_penalty)
        return kw if self.sampling is not None else dict(kw, unk=self.unk, unk_penalty=self.unk_penalty)

    def _row_pass(self, logits, t, dec, st, max_len, ngram, ctx):
        """The step's row pass into st["ws"]; returns the vocabulary width the sentence pass works with."""
        K.beam_topk(logits, self.beam_size, t, st["ws"], **self._policy(dec, st, max_len, ngram))
        return logits.shape[1]

    def _sentence_pass(self, t, st, V, max_len):
        """The step's sentence pass over st["ws"]: plain beam search, or the diverse strategy's over the same candidates."""
        if isinstance(self.diverse, DiverseBeamSearch):
            K.diverse_group_select(st["ws"], st, self.beam_size, V, t, max_len, self.diverse.num_groups,
                                   self.diverse.diversity_strength, **self._select())
        elif isinstance(self.diverse, DiverseSiblingsSearch):
            K.diverse_sibling_select(st["ws"], st, self.beam_size, V, t, max_len, self.diverse.diversity_rate, **self._select())
        else:
            K.beam_select(st["ws"], st, self.beam_size, V, t, max_len, **self._select())

    def _advance(self, t, st, ctx):
        """Device work between the sentence pass and the cache reorder."""

    def _prefix_step_kernels(self, out, t, dec, st, max_len, forced):
        """A step of a sample whose prefix has columns.  forced: a prefix step (t < width and t < max_len) -- the row pass without
        the min_len mask and without candidates for forced rows, the fill, and the sentence pass told which rows are normalised.
        Otherwise a free step: the plain two launches, with the n-gram bans following the prefix lengths."""
        beam, V = self.beam_size, out.shape[1]
        policy = self._policy(dec, st, max_len, self.no_repeat_ngram_size)
        K.beam_prefix_topk(out, beam, t, st["ws"], st["plen"], prefix=st["prefix"] if forced else None, glogit=st["glogit"], **policy)
        st["tokens"] = dec.tokens
        if forced:
            K.beam_prefix_fill(st["ws"], out.shape[0], V, beam, t, st["prefix"], st["plen"], st["glogit"], **policy)
            K.beam_prefix_select(st["ws"], st, beam, V, t, max_len, st["prefix"], pad=self.pad, **self._select())
        else:
            K.beam_select(st["ws"], st, beam, V, t, max_len, **self._select())
        dec.reorder(st["reorder"], caches_only=True)

    def _step_kernels(self, out, t, dec, st, max_len, ngram_step0=True, ctx=None):
        """Everything a step does after the decoder, on the device (recorded into the step graph)."""
        ngram = self.no_repeat_ngram_size if (t > 0 or ngram_step0) else 0
        if self.sampling is not None:
            return self._sample_step_kernels(out, t, dec, st, max_len, ngram)
        V = self._row_pass(out, t, dec, st, max_len, ngram, ctx)
        st["tokens"] = dec.tokens
        self._sentence_pass(t, st, V, max_len)
        self._advance(t, st, ctx)
        dec.reorder(st["reorder"], caches_only=True)

    def _sample_step_kernels(self, out, t, dec, st, max_len, ngram):
        """A sampling step: every row's draw from row t of the uniforms, then the K-wide sentence pass."""
        K.sample_draw(out, self.beam_size, t, st["sample_ws"], st["uniforms"][t], topk=self.sampling.sampling_topk,
                      topp=self.sampling.sampling_topp, **self._policy(dec, st, max_len, ngram))
        st["tokens"] = dec.tokens
        K.sample_select(st["sample_ws"], st, self.beam_size, t, max_len, **self._select())
        dec.reorder(st["reorder"], caches_only=True)

    def _fill_uniforms(self, st, uniforms):
        """One number in [0, 1) per (step, row): the caller's table, or one launch of a generator seeded once -- from `seed`, or
        from torch's global generator -- so successive generate() calls draw on."""
        buf = st["uniforms"]
        if uniforms is not None:
            if tuple(uniforms.shape) != tuple(buf.shape):
                raise ValueError(f"generate: uniforms must be [steps + 1, rows] = {tuple(buf.shape)}, got {tuple(uniforms.shape)}")
            buf.copy_(uniforms.to(torch.float32))
            return
        if self._rng is None or self._rng.device != buf.device:
            self._rng = torch.Generator(device=buf.device)
            self._rng.manual_seed(int(torch.randint(0, 2 ** 62, (1,)).item()) if self.seed is None else int(self.seed))
        buf.uniform_(generator=self._rng)

    # ------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, model, sample, uniforms=None, **kwargs):
        """uniforms (sampling only): fp32 [steps + 1, rows], row t the numbers of step t -- the draws are a function of them."""
        if uniforms is not None and self.diverse is not None:
            raise NotImplementedError("generate: uniforms together with a diverse search strategy are not implemented (they are "
                                      "read by sampling only)")
        if uniforms is not None and self.sampling is None:
            raise ValueError("generate: uniforms are read by sampling only (search_strategy=Sampling(...))")
        ngram_step0 = self.check_sample(sample, **kwargs)
        prefix = self._prefix_of(sample)
        source_slots = [s for s in sample["net_input"]["slots"] if s.is_src]
        first = source_slots[0].value
        src = first["fbank"] if isinstance(first, dict) else first
        bsz, device = src.shape[0], src.device
        beam = self.beam_size
        rows = bsz * beam
        max_len = self.effective_max_len(sample)
        assert self.min_len <= max_len, "min_len cannot be larger than max_len, please adjust these!"
        steps, V, ctx = self._setup(model, max_len, device)
        dec = self._decoder(model, steps + 1)
        dec.begin(source_slots, torch.arange(bsz, device=device).repeat_interleave(beam))
        dec.tokens.fill_(self.pad)
        dec.tokens[:, 0] = self.bos
        st = self._buffers(rows, bsz, V, steps, device)
        if self.sampling is not None:
            self._fill_uniforms(st, uniforms)
        post = lambda out, t: self._step_kernels(out, t, dec, st, max_len, ngram_step0, ctx)   # noqa: E731
        variant = None
        if prefix is not None:
            tok, plen = prefix
            width = min(tok.size(1), max_len)                 # prefix steps: t < tok.size(1) and t < max_len
            st["prefix"].fill_(self.pad)
            st["prefix"][:, :width] = tok[:, :width]
            st["plen"].copy_(plen)
            post = lambda out, t: self._prefix_step_kernels(out, t, dec, st, max_len, t < width)   # noqa: E731
            variant = lambda t: "prefix" if t < width else "free after a prefix"               # noqa: E731
        self._loop(dec, st, bsz, steps + 1, post, self._check_output, variant)
        return self._collect(st, bsz)

    def _loop(self, dec, st, bsz, nsteps, post, check=None, variant=None):
        """At most `nsteps` decoding steps, stopping once every sentence is finished.  variant(step): what distinguishes this
        sequence's `post` at that step from another sequence's (the key of the step's graph)."""
        host, events = st["host"], [None, None]
        for step in range(nsteps):
            out = dec.step(None, post=post, variant=None if variant is None else variant(step))
            if check is not None:
                check(out)
            # the all-finished counter reaches the host one step late, through pinned memory: no synchronisation inside a step
            host[step % 2].copy_(st["nfin"][0], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            events[step % 2] = ev
            self.steps_run = step + 1
            if step > 0:
                events[(step - 1) % 2].synchronize()
                if int(host[(step - 1) % 2]) >= bsz:
                    break
        torch.cuda.synchronize()

    def _collect(self, st, bsz):
        cnt, ln = st["fin_cnt"].cpu(), st["fin_len"].cpu()
        toks, pos, sc = st["fin_tok"].cpu(), st["fin_pos"].cpu(), st["fin_score"].cpu()
        out = []
        for b in range(bsz):
            hyps = [SequenceGeneratorOutput(tokens=toks[b, i, :int(ln[b, i])].clone(), score=sc[b, i].clone(),
                                            attention=torch.empty(0), positional_scores=pos[b, i, :int(ln[b, i])].clone())
                    for i in range(int(cnt[b]))]
            scores = torch.tensor([float(h.score.item()) for h in hyps])
            _, order = torch.sort(scores, descending=True)
            if self.return_n_best == 1:
                out.append(hyps[order[0]])
            else:
                out.append([hyps[i] for i in order][: self.return_n_best])
        return out


class TrieBeamGenerator(SequenceGenerator):
    """Beam search over the answer trie of a closed set: `plan` is a traverse.TraversePlan; the options, defaults and refusals are
    SequenceGenerator's.  Every step is restricted to the children of the trie node a row has reached, as the reference's generator
    does with a `constraint_trie` -- so `constraint_range` cannot be given as well (the reference asserts it, :730), and a
    `prefix_tokens` with columns stays refused (its prefix steps need the full-vocabulary normaliser).

    The row pass never forms [rows, V] logits: the decoder returns features and csrc/trie_beam.hip computes one dot product per
    child edge.  The decoder's capacity and the step loop follow min(max_len, plan.Tmax) -- no hypothesis is longer than the deepest
    answer -- and a sentence stops as soon as nothing more can be finalised, where the reference runs its remaining steps on
    all -inf rows.  Beam search is not the exact arg-max over the closed set (TraverseTask.score is)."""

    def __init__(self, tgt_dict, plan, *args, **kwargs):
        if kwargs.get("constraint_range") is not None:
            raise ValueError("TrieBeamGenerator: constraint_range cannot be combined with a constraint trie")
        if isinstance(kwargs.get("search_strategy"), (DiverseBeamSearch, DiverseSiblingsSearch)):
            raise NotImplementedError("TrieBeamGenerator: a diverse search strategy over the answer trie is not implemented "
                                      "(search_strategy must be None)")
        if kwargs.get("search_strategy") is not None:
            raise NotImplementedError("TrieBeamGenerator: only beam search is implemented (search_strategy must be None)")
        super().__init__(tgt_dict, *args, **kwargs)
        if (plan.bos, plan.eos, plan.pad) != (self.bos, self.eos, self.pad):
            raise ValueError("TrieBeamGenerator: the plan was built with other BOS / EOS / PAD ids than the dictionary's")
        self.plan = plan
        self._dev: Dict[torch.device, Dict[str, object]] = {}

    def _prefix_of(self, sample):
        prefix = sample.get("prefix_tokens")
        if prefix is not None and prefix.dim() == 2 and prefix.size(1) > 0:
            raise NotImplementedError("TrieBeamGenerator: prefix_tokens are not implemented (got a prefix of "
                                      f"{prefix.size(1)} columns)")
        return None

    def _plan_on(self, device):
        if device not in self._dev:
            self._dev[device] = self.plan.to_device(device)
        return self._dev[device]

    def _buffers(self, rows, bsz, V, max_len, device):
        fresh = self._state is None or self._state["key"] != (rows, V, max_len, device)
        st = super()._buffers(rows, bsz, V, max_len, device)
        if fresh:
            st["node"] = torch.zeros(rows, dtype=torch.int32, device=device)
        st["node"].zero_()                                # every row starts at the root
        return st

    def _setup(self, model, max_len, device):
        from .traverse import TraverseTask
        weight, bias = TraverseTask.output_projection(model)
        V = weight.shape[0]
        if V > self.vocab_size:
            raise ValueError(f"decoder output width {V} > dictionary size {self.vocab_size}")
        if int(self.plan.edge_token.max()) >= V:
            raise ValueError(f"the closed set holds token id {int(self.plan.edge_token.max())}, the output projection has {V} rows")
        # no hypothesis is longer than the deepest answer (+ EOS)
        return min(max_len, self.plan.Tmax), V, (self._plan_on(device), weight, bias)

    def _decoder(self, model, capacity):
        if self._dec is None or self._dec.model is not model or self._dec.max_len != capacity:
            self._dec = StepDecoder(model, capacity, use_graph=self.use_graph, features_only=True)
        return self._dec

    def _check_output(self, feats):
        pass                                              # features [rows, D]: the projection's width was checked in _setup

    def _row_pass(self, feats, t, dec, st, max_len, ngram, ctx):
        dev, weight, bias = ctx
        if feats.dtype != weight.dtype:
            feats = feats.to(weight.dtype)
        K.trie_beam_topk(feats, weight, bias, dev, st["node"], self.beam_size, t, st["ws"], **self._policy(dec, st, max_len, ngram))
        return weight.shape[0]

    def _advance(self, t, st, ctx):
        K.trie_beam_advance(ctx[0], st["node"], st, self.beam_size, t)

    def _collect(self, st, bsz):
        if self.return_n_best == 1:                       # (the reference indexes an empty list here)
            empty = (st["fin_cnt"].cpu() == 0).nonzero().flatten().tolist()
            if empty:
                raise ValueError(f"TrieBeamGenerator: no finalised hypothesis for sentence {empty[0]} of the batch "
                                 f"(beam {self.beam_size}, min_len {self.min_len}, max_len {self.max_len}: no answer of the closed "
                                 "set survives the length limits and the beam)")
        return super()._collect(st, bsz)


# ---------------------------------------------------------------------------------------------------------------- speech generation
def _to_numpy(x):
    return x.detach().cpu().float().numpy() if torch.is_tensor(x) else x


@dataclass
class SpeechGeneratorOutput:
    """One generated utterance (generator/speech_generator.py:25-54): the denormalised frames [out_len, raw_dim], the end-of-sequence
    probability of every frame, the head-averaged cross-attention of the alignment layer [S, out_len] with its arg-max per frame, and
    with `has_targ` the target's frames.  `waveform` / `text` stay None: the vocoder is out of scope."""
    feature: Any
    eos_prob: torch.Tensor
    attn: torch.Tensor
    alignment: torch.Tensor
    text: Optional[str] = None
    waveform: Any = None
    targ_feature: Any = None
    targ_waveform: Any = None

    def save_audio(self, audio_name: str, sample_rate: int = 22050, target: bool = False):
        import soundfile as sf                                  # (only needed here; absent: ImportError)
        waveform = _to_numpy(self.targ_waveform if target else self.waveform)
        assert waveform is not None
        if not audio_name.endswith(".wav"):
            audio_name = audio_name + ".wav"
        sf.write(audio_name, waveform, sample_rate)

    def save_fbank(self, fbank_name: str, target: bool = False):
        import numpy as np
        feature = _to_numpy(self.targ_feature if target else self.feature)
        assert feature is not None
        if not fbank_name.endswith(".npy"):
            fbank_name = fbank_name + ".npy"
        np.save(fbank_name, feature)


class SpeechGenerator:
    """Base generator of the AUDIO modality (generator/speech_generator.py:57-81).  stats_npz_path: a LOCAL .npz holding the global
    cepstral mean / variance statistics `mean` and `std` [raw_dim] (the reference also takes URLs; nothing here fetches one)."""

    def __init__(self, src_dict, stats_npz_path: Optional[str] = None):
        self.pad, self.unk, self.bos, self.eos = src_dict.pad(), src_dict.unk(), src_dict.bos(), src_dict.eos()
        self.gcmvn_stats = None
        if stats_npz_path is not None:
            import numpy as np
            with np.load(stats_npz_path) as f:
                self.gcmvn_stats = {"mean": f["mean"], "std": f["std"]}

    def gcmvn_denormalize(self, x):
        """x [B, T, C] -> x * std + mean (the identity without statistics)."""
        if self.gcmvn_stats is None:
            return x
        mean = torch.from_numpy(self.gcmvn_stats["mean"]).to(x)
        std = torch.from_numpy(self.gcmvn_stats["std"]).to(x)
        assert len(x.shape) == 3 and mean.shape[0] == std.shape[0] == x.shape[2]
        x = x * std.view(1, 1, -1).expand_as(x)
        return x + mean.view(1, 1, -1).expand_as(x)


class SpeechStepDecoder(StepDecoder):
    """StepDecoder for an [AUDIO:fbank] target: a step feeds the decoder ONE embedded frame through the audio adaptor's step form
    (adaptor/audio.py forward_step) instead of a token prefix, returns the new position's features [B, D] and keeps the head-averaged
    cross-attention row of the alignment layer in `state["attn"][:, t]`.  The buffers a step reads and writes (`state`, see
    kernels.speech_step) sit at fixed addresses for the step graphs; steps from `graph_cap` on run eagerly (a captured
    step costs device memory, and max_iter is in the thousands)."""

    def __init__(self, model, max_len: int, target_slot: Slot, use_graph: bool = True, graph_cap: Optional[int] = None):
        super().__init__(model, max_len, use_graph=use_graph, features_only=True)
        self.graph_cap = self.max_len if graph_cap is None else int(graph_cap)
        self.adaptor = model.decoder.adaptor.get_adaptor(target_slot)
        self.attributes = target_slot.attributes
        self.state: Optional[Dict[str, torch.Tensor]] = None
        self._state_inc = None

    def begin(self, src_slots: List[Slot], beam_order: Optional[torch.Tensor] = None):
        super().begin(src_slots, beam_order)
        rows, dtype, dev = self._shape[0], self._shape[2], self.tokens.device
        ad = self.adaptor
        if self._state_inc is not self.inc:                 # another batch shape (or other parameters): new buffers
            i32 = dict(dtype=torch.int32, device=dev)
            self.state = {
                "feats": torch.zeros(rows, self.max_len, ad.out_dim, dtype=dtype, device=dev),
                "eos_prob": torch.zeros(rows, self.max_len, dtype=torch.float32, device=dev),
                "attn": torch.zeros(rows, self.max_len, self._shape[1], dtype=torch.float32, device=dev),
                "finished": torch.zeros(rows, **i32), "out_lens": torch.zeros(rows, **i32), "nfin": torch.zeros(1, **i32),
                "pad_next": torch.zeros(rows, 1, dtype=torch.bool, device=dev),
                "embed": torch.zeros(rows, ad.cfg.embed_dim, dtype=dtype, device=dev),
                "threshold": torch.zeros(1, dtype=torch.float32, device=dev),
                "host": torch.zeros(2, dtype=torch.int32, pin_memory=True),
            }
            self._state_inc = self.inc
        st = self.state
        for name in ("finished", "nfin", "pad_next"):
            st[name].zero_()
        st["out_lens"].fill_(self.max_len)
        with torch.no_grad():                               # position 0 is fed a zero frame (generator/speech_generator.py:142)
            st["embed"].copy_(ad.embed_frame(torch.zeros(rows, ad.out_dim, dtype=dtype, device=dev)))
        from . import ops
        ops.rng_advance()
        return self

    def step(self, next_tokens=None, post=None, variant=None):
        if self.use_graph and self.t >= self.graph_cap:     # beyond the cap: eagerly (the host-side cache lengths follow either way)
            self.use_graph = False
            try:
                return super().step(next_tokens, post=post, variant=variant)
            finally:
                self.use_graph = True
        return super().step(next_tokens, post=post, variant=variant)

    def _run(self, t):
        st = self.state
        rows = st["embed"].shape[0]
        slot = Slot(ModalityType.AUDIO, False, {"frame_embed": st["embed"].view(rows, 1, -1), "step": t, "padded": st["pad_next"]},
                    attributes=self.attributes)
        out, extra = self.model.decoder([slot], encoder_out=self.enc, incremental_state=self.inc, features_only=True)
        st["attn"][:, t].copy_(extra["attn"][0][:, 0])      # [B, 1, S]: the new position's row
        return out[:, -1]


class AutoRegressiveSpeechGenerator(SpeechGenerator):
    """The reference's autoregressive generator of fbank frames (generator/speech_generator.py:84-200) on `SpeechStepDecoder`: a step
    is the decoder on ONE new position plus one launch (csrc/speech_step.hip: head, sigmoid, finish rule, next padding flag, finished
    count, prenet of the new frame), recorded into the step's hipGraph -- no host synchronisation inside a step; the all-finished
    count reaches the host one step late (`SequenceGenerator._loop`) and the step that may have run in excess is cut off before the
    postnet.  Semantics are the reference's: the finish test is strict, finished rows keep decoding (their later positions are padded
    keys of their own cache, their later frames are fed back and reach their kept frames through the postnet's window), rows that
    never finish keep max_iter.  Differences ("Speech generation"): `attn` holds every step's map, results are on
    the CPU, no waveform, a local statistics file.  fused_step=False (or a shape the kernel does not serve) runs the step's policy as
    the unfused composition of the existing kernels; `fused` reports which ran."""

    def __init__(self, src_dict, stats_npz_path: Optional[str] = None, max_iter: int = 6000, eos_prob_threshold: float = 0.5,
                 use_graph: bool = True, fused_step: bool = True, graph_cap: Optional[int] = 512, **unused_kwargs):
        super().__init__(src_dict, stats_npz_path)
        self.max_iter, self.eos_prob_threshold = int(max_iter), float(eos_prob_threshold)
        self.use_graph, self.fused_step, self.graph_cap = use_graph, bool(fused_step), graph_cap
        self.fused: Optional[bool] = None                   # which step path the last generate() ran
        self.steps_run = 0
        self._dec: Optional[SpeechStepDecoder] = None

    def check_limits(self, model, audio_adaptor):
        """max_iter against what the model can address, before anything runs."""
        for limit, what in ((audio_adaptor.embed_audio_positions.weight.shape[0], "embed_audio_positions"),
                            (audio_adaptor.audio_rp_bucket.size(0), "audio_rp_bucket"),
                            (model.decoder.max_positions(), "the decoder's max_target_positions")):
            if self.max_iter > int(limit):
                raise ValueError(f"AutoRegressiveSpeechGenerator: max_iter={self.max_iter} exceeds {what} ({int(limit)})")

    @torch.no_grad()
    def generate(self, model, sample, has_targ: bool = False, **kwargs):
        from . import ops
        model.eval()
        net_input = sample["net_input"]
        source_slots = [s for s in net_input["slots"] if s.is_src]
        target_slot = Slot.get_target_slot_from_slots(net_input["slots"])
        assert target_slot.modality == ModalityType.AUDIO, (
            f"the target slot does not match the generator,"
            f" target_slot: {target_slot.modality}, generator: AutoRegressiveSpeechGenerator")
        ad = model.decoder.adaptor.get_adaptor(target_slot)
        self.check_limits(model, ad)
        first = source_slots[0].value
        src = first["fbank"] if isinstance(first, dict) else first
        bsz = src.shape[0]
        n, out_dim = ad.n_frames_per_step, ad.out_dim
        raw_dim = out_dim // n

        if self._dec is None or self._dec.model is not model or self._dec.adaptor is not ad or self._dec.max_len != self.max_iter:
            self._dec = SpeechStepDecoder(model, self.max_iter, target_slot, use_graph=self.use_graph, graph_cap=self.graph_cap)
        dec = self._dec
        dec.begin(source_slots)
        st = dec.state
        head, prenet, proj = ad.step_weights()
        p_drop = float(ad.prenet[0].dropout)
        self.fused = self.fused_step and ops.speech_step_fusable(st["embed"].dtype, head, prenet, proj)

        def post(out, t):
            ops.speech_step(out, head, prenet, proj, st, t, p_drop, fused=self.fused)
            if p_drop > 0:
                ops.rng_advance()                           # (captured: a replayed step moves the Philox position on the device)

        st["threshold"].fill_(self.eos_prob_threshold)      # read on the device: a captured step serves every threshold
        variant = ("fused" if self.fused else "unfused", p_drop)
        SequenceGenerator._loop(self, dec, st, bsz, self.max_iter, post, None, lambda step: variant)

        out_lens = st["out_lens"].cpu().long()
        T_run = int(out_lens.max())                         # the steps the reference runs; one more may have run here: cut it off
        assert T_run <= self.steps_run
        feat = st["feats"][:, :T_run].contiguous()
        feat = ad.postnet(feat, residual=feat)              # eval mode: running statistics, no dropout; over the padded [B, T_run]
        eos_prob = st["eos_prob"][:, :T_run]
        attn = st["attn"][:, :T_run].transpose(1, 2)        # [B, S, T_run]
        alignment = attn.max(dim=1)[1]
        feat = self.gcmvn_denormalize(feat.reshape(bsz, -1, raw_dim))
        eos_prob = eos_prob.repeat_interleave(n, dim=1).cpu()
        attn = attn.repeat_interleave(n, dim=2).cpu()
        alignment = alignment.repeat_interleave(n, dim=1).cpu()
        out_lens = out_lens * n
        feat = feat.cpu()
        finalized = [SpeechGeneratorOutput(feature=feat[b, :l].clone(), eos_prob=eos_prob[b, :l].clone(), attn=attn[b, :, :l].clone(),
                                           alignment=alignment[b, :l].clone()) for b, l in enumerate(out_lens.tolist())]
        if has_targ:
            assert sample["target"].size(-1) == out_dim
            tgt_feats = self.gcmvn_denormalize(sample["target"].view(bsz, -1, raw_dim))
            tgt_lens = (sample["target_lengths"] * n).tolist()
            for b, (f, l) in enumerate(zip(tgt_feats, tgt_lens)):
                finalized[b].targ_feature = f[:l].cpu()
        return finalized
