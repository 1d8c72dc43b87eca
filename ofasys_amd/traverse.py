"""Closed-set inference (reference: task/traverse_task.py, exported as `ofasys.task.TraverseTask`): score every answer of a
closed set under teacher forcing, each position's distribution restricted to the answer trie's next layer, and return the best
answer.  The route for the tasks `Task.generator` refuses (an instruction whose target carries `closed_set`: VQA with an answer
list, classification, SNLI-VE).  `search="beam"` is the reference's everyday route for the same tasks instead: beam search whose
every step is restricted to the trie's next layer (generator.TrieBeamGenerator) -- sentences x beam decoder rows for at most
longest answer + 1 steps whatever the size of the closed set, but not the exact arg-max.

The reference projects every (answer, position) onto the vocabulary, masks, takes a full log-softmax and gathers.  Here the trie is
flattened once on the host (`TraversePlan`) and the device computes one dot product per trie EDGE, one log-sum-exp per trie NODE
and one short sum per answer (csrc/closed_set_score.hip); the [rows, T, V] logits never exist.  The decoder still runs per answer
(features only), in chunks of answers so that memory does not grow with the size of the closed set.
"""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import criterion
from . import kernels as K
from .preprocessor import ModalityType, Slot
from .task import Task


class TraversePlan:
    """The answer trie as flat int32 arrays.  `answers`: token-id sequences without BOS / EOS, in label order.

    nodes        distinct prefixes [bos] + answer[:t], t = 0 .. len, numbered in order of first appearance (node 0 = [bos]); so the
                 nodes first reached by answers c0 .. c1 - 1 are one contiguous range, and so are their edges and work items
    edges        CSR by node: node_edge_off [N + 1], edge_token [E], edge_node [E]; an answer's last edge is EOS.  edge_child [E] is
                 the node an edge leads to (-1 for an EOS edge) and max_degree the largest number of edges of one node: what the
                 trie-constrained beam search walks (csrc/trie_beam.hip)
    rep_ans/pos  [N] the lowest answer index passing through the node and the position t: the decoder row holding its state
    paths        path_off [C + 1], path_edge [P]: the len + 1 edges of every answer
    items        [I, 3] (node, first edge, one past the last): the edges in pieces of at most ITEM_EDGES edges of one node -- the
                 unit of work of the edge kernel (the root's ~C edges spread over C / ITEM_EDGES workgroups)
    prev_output_tokens / target   [C, Tmax] as traverse_task.py:32-61 pads them (BOS first / EOS last, <pad> after)
    """

    ITEM_EDGES = 8

    def __init__(self, answers: Sequence[Sequence[int]], bos: int, eos: int, pad: int):
        answers = [[int(t) for t in a] for a in answers]
        if len(answers) == 0:
            raise ValueError("TraversePlan: the closed set is empty")
        self.C = C = len(answers)
        self.bos, self.eos, self.pad = int(bos), int(eos), int(pad)
        self.lengths = np.array([len(a) + 1 for a in answers], np.int32)
        self.Tmax = T = int(self.lengths.max())
        self.prev_output_tokens = np.full((C, T), pad, np.int64)
        self.target = np.full((C, T), pad, np.int64)
        node_of = {(): 0}
        rep = [(0, 0)]
        children: List[Dict[int, int]] = [{}]                # node -> {token: child node or -1 (EOS)}, insertion order as Trie
        for c, a in enumerate(answers):
            self.prev_output_tokens[c, :len(a) + 1] = [bos] + a
            self.target[c, :len(a) + 1] = a + [eos]
            for t in range(1, len(a) + 1):
                key = tuple(a[:t])
                if key not in node_of:
                    node_of[key] = len(rep)
                    rep.append((c, t))
                    children.append({})
                children[node_of[tuple(a[:t - 1])]].setdefault(a[t - 1], node_of[key])
            children[node_of[tuple(a)]].setdefault(eos, -1)
        self.N = N = len(rep)
        self.rep_ans = np.array([r[0] for r in rep], np.int32)
        self.rep_pos = np.array([r[1] for r in rep], np.int32)
        self.node_edge_off = np.zeros(N + 1, np.int32)
        self.node_edge_off[1:] = np.cumsum([len(ch) for ch in children])
        self.E = E = int(self.node_edge_off[-1])
        self.edge_token = np.array([tok for ch in children for tok in ch], np.int32)
        self.edge_node = np.repeat(np.arange(N, dtype=np.int32), np.diff(self.node_edge_off))
        self.edge_child = np.array([child for ch in children for child in ch.values()], np.int32)
        self.max_degree = int(np.diff(self.node_edge_off).max())
        edge_of = [{tok: int(self.node_edge_off[n]) + i for i, tok in enumerate(ch)} for n, ch in enumerate(children)]
        self.path_off = np.zeros(C + 1, np.int32)
        self.path_off[1:] = np.cumsum(self.lengths)
        path = []
        for a in answers:
            for t, tok in enumerate(a + [eos]):
                path.append(edge_of[node_of[tuple(a[:t])]][tok])
        self.path_edge = np.array(path, np.int32)
        self.P = len(path)
        items = []
        for n in range(N):
            lo, hi = int(self.node_edge_off[n]), int(self.node_edge_off[n + 1])
            items.extend((n, e, min(e + self.ITEM_EDGES, hi)) for e in range(lo, hi, self.ITEM_EDGES))
        self.items = np.array(items, np.int32).reshape(-1, 3)
        self.head_tokens, self.tok_edge_off, self.tok_edge = self.invert_edges(self.edge_token)
        self.U = len(self.head_tokens)
        self._child_of = None                               # walk()'s (node, token) -> child map, built on first use
        assert E == len(self.edge_token) == len(self.edge_node) and int(self.path_off[-1]) == self.P

    @staticmethod
    def invert_edges(edge_token):
        """The inverse CSR by token of an edge list: (head_tokens [U] the distinct tokens, ascending; tok_edge_off [U + 1]; tok_edge [E]
        the edge indices, ascending within a token), int32.  One token can hang under many nodes; the trie-edge head's weight
        gradient (csrc/trie_head.hip) gives each distinct token to one wave, which walks that token's edges in this order."""
        edge_token = np.asarray(edge_token, np.int32)
        order = np.argsort(edge_token, kind="stable").astype(np.int32)              # by token, then by edge index
        tokens, counts = np.unique(edge_token, return_counts=True)
        off = np.zeros(len(tokens) + 1, np.int32)
        off[1:] = np.cumsum(counts)
        return tokens.astype(np.int32), off, order

    def allowed(self, c: int, t: int) -> List[int]:
        """The tokens position t of answer c may take: Trie.get_next_layer(prev_output_tokens[c, :t + 1])."""
        n = self.node_of(c, t)
        return self.edge_token[self.node_edge_off[n]:self.node_edge_off[n + 1]].tolist()

    def node_of(self, c: int, t: int) -> int:
        """The node reached by the first t tokens of answer c (t <= its length): the node of its t-th path edge."""
        return int(self.edge_node[self.path_edge[self.path_off[c] + t]])

    def walk(self, tokens) -> np.ndarray:
        """int32 [len(tokens) + 1]: entry i is the node reached by tokens[:i] (node 0 for the empty prefix), so the children of entry i
        are the tokens position i may take and the last entry is the node whose edge is EOS.  `tokens`: an answer of the closed set
        without BOS / EOS; a token that is no child of the node reached so far raises ValueError (the reference's loss for such a
        sample is +inf: the target's log-probability is masked to -inf)."""
        if self._child_of is None:                            # (node, token) -> child, once
            node = np.repeat(np.arange(self.N), np.diff(self.node_edge_off))
            self._child_of = {(int(n), int(t)): int(c) for n, t, c in zip(node, self.edge_token, self.edge_child)}
        tokens = [int(t) for t in tokens]
        out = np.zeros(len(tokens) + 1, np.int32)
        n = 0
        for i, t in enumerate(tokens):
            child = self._child_of.get((n, t), -1)
            if child < 0:                                     # not a child at all, or EOS in the middle of an answer
                raise ValueError(f"TraversePlan.walk: token {t} at position {i} of {tokens} is not a child of the trie node its "
                                 f"prefix reaches: the answer is outside the closed set")
            out[i + 1] = n = child
        if (n, self.eos) not in self._child_of:
            raise ValueError(f"TraversePlan.walk: {tokens} ends at position {len(tokens)} on a node without an EOS edge: the answer "
                             f"is outside the closed set (a strict prefix of one of its answers)")
        return out

    def chunk_items(self, c0: int, c1: int):
        """The rows [i0, i1) of `items` whose node is represented by an answer in [c0, c1), and the chunk's longest row."""
        n0, n1 = np.searchsorted(self.rep_ans, [c0, c1], side="left")        # rep_ans is non-decreasing
        i0, i1 = np.searchsorted(self.items[:, 0], [n0, n1], side="left")
        return int(i0), int(i1), int(self.lengths[c0:c1].max())

    def to_device(self, device) -> Dict[str, object]:
        """The arrays the kernels read (kernels.closed_set_*), on `device`, plus the padded decoder inputs."""
        d = {k: torch.from_numpy(getattr(self, k)).to(device) for k in
             ("node_edge_off", "edge_token", "edge_node", "rep_ans", "rep_pos", "path_off", "path_edge", "items",
              "prev_output_tokens", "edge_child", "head_tokens", "tok_edge_off", "tok_edge")}
        d.update(C=self.C, N=self.N, E=self.E, P=self.P, Tmax=self.Tmax, max_degree=self.max_degree, U=self.U)
        return d

    def head_arrays(self, device) -> Dict[str, object]:
        """What the node criterion and the trie-edge head read, on `device`: the CSR by node (node_edge_off, edge_token, edge_node), the
        inverse CSR by token (head_tokens, tok_edge_off, tok_edge), node_ids = arange(N + 1) (the per-step row buckets search it) and
        the ints N, E, U, max_degree."""
        d = {k: torch.from_numpy(getattr(self, k)).to(device) for k in
             ("node_edge_off", "edge_token", "edge_node", "head_tokens", "tok_edge_off", "tok_edge")}
        d["node_ids"] = torch.arange(self.N + 1, dtype=torch.int32, device=device)
        d.update(N=self.N, E=self.E, U=self.U, max_degree=self.max_degree)
        return d


class TraverseTask(Task):
    """`Task` for closed-set targets.  `max_rows`: cap on the decoder rows (sentences x answers) of one chunk; the answers are
    processed `max(1, max_rows // bsz)` at a time, so device memory follows the cap and not the size of the closed set.  The
    default, 2048 rows, keeps the decoder's GEMMs at a few thousand rows x Tmax -- large enough to fill the device at OFA-base
    size, while activations stay in the tens of MB.
    `search`: what `inference` does by default -- "all" scores every answer (exact), "beam" runs the trie-constrained beam search with
    `beam` beams (`beam_search`)."""

    SEARCHES = ("all", "beam")

    def __init__(self, cfg=None, max_rows: int = 2048, search: str = "all", beam: int = 5, **kwargs):
        super().__init__(cfg, **kwargs)
        if max_rows < 1:
            raise ValueError("TraverseTask: max_rows must be >= 1")
        if search not in self.SEARCHES:
            raise ValueError(f"TraverseTask: search must be one of {self.SEARCHES}, got {search!r}")
        if beam < 1:
            raise ValueError("TraverseTask: beam must be >= 1")
        self.max_rows, self.search, self.beam = int(max_rows), search, int(beam)
        self._seq2label: Dict[tuple, int] = {}
        self._trie_gens: Dict[tuple, object] = {}
        self.plan: Optional[TraversePlan] = None
        self.index2ans: Dict[int, object] = {}
        self._dev: Dict[torch.device, Dict[str, object]] = {}
        self._buf: Dict[tuple, Dict[str, torch.Tensor]] = {}

    def initialize(self, global_dict, closed_set=None, **kwargs):
        """As Task.initialize, then the plan of the text preprocessor's closed set: `closed_set` (answer strings or token-id
        sequences, a list or a dict answer -> label), else cfg.text.ans2label, else what an earlier initialize + the text
        preprocessor's prepare_for_generation left."""
        before = self.general_preprocess.name2pre["text"].ans2label_dict if self.general_preprocess is not None else None
        super().initialize(global_dict, **kwargs)
        pre = self.general_preprocess.name2pre["text"]
        if closed_set is None and not pre.ans2label_dict:
            closed_set = before
        if closed_set is not None:
            pre.prepare_for_generation(closed_set)
        if not pre.ans2label_dict:
            raise ValueError(f"task {self.name}: TraverseTask needs a closed set -- pass initialize(global_dict, closed_set=[...]), "
                             "set cfg.text.ans2label to the JSON of an answer -> label dict, or call the text preprocessor's "
                             "prepare_for_generation(closed_set) and initialize again")
        self.build_plan()

    def build_plan(self):
        pre, d = self.general_preprocess.name2pre["text"], self.global_dict
        answers = list(pre.ans2label_dict.keys() if isinstance(pre.ans2label_dict, dict) else pre.ans2label_dict)
        self.index2ans = dict(enumerate(answers))
        ids = [pre.encode(a).tolist() if isinstance(a, str) else [int(t) for t in a] for a in answers]
        if any(t < 0 or t >= len(d) for a in ids for t in a):
            raise ValueError(f"task {self.name}: the closed set holds token ids outside the dictionary (size {len(d)})")
        # (closed_set_nodes: the text preprocessor already holds the plan of these answers for its collation -- one object, not two)
        self.plan = pre.constraint_plan if pre.constraint_plan is not None else TraversePlan(ids, d.bos(), d.eos(), d.pad())
        self._dev, self._buf, self._trie_gens = {}, {}, {}
        self._seq2label = {}
        for i, a in enumerate(ids):                           # duplicates go to the lowest label
            self._seq2label.setdefault(tuple(a), i)

    # ------------------------------------------------------------------ device state
    def _plan_on(self, device):
        if device not in self._dev:
            self._dev[device] = self.plan.to_device(device)
        return self._dev[device]

    def _buffers(self, bsz, device):
        key = (bsz, device)
        if key not in self._buf:                              # the pass's own scratch: allocated eagerly, never inside a capture
            n = (K.closed_set_ws_bytes(bsz, self.plan.E, self.plan.N) + 3) // 4
            self._buf[key] = {"ws": torch.empty(n, dtype=torch.float32, device=device),
                              "scores": torch.empty(bsz, self.plan.C, dtype=torch.float32, device=device)}
        return self._buf[key]

    output_projection = staticmethod(criterion.output_projection)

    # ------------------------------------------------------------------ scoring (traverse_task.py:63-110)
    @torch.no_grad()
    def score(self, model, sample) -> torch.Tensor:
        """log p(answer | source) under the trie constraint for every answer: float32 [bsz, C] on the CPU."""
        if self.plan is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) first")
        model.eval()
        plan = self.plan
        src = [s for s in sample["net_input"]["slots"] if s.is_src]
        enc = model.encoder(src)
        out = enc["encoder_out"][0]
        bsz, device = out.shape[1], out.device
        dev, buf = self._plan_on(device), self._buffers(bsz, device)
        weight, bias = self.output_projection(model)
        if int(plan.edge_token.max()) >= weight.shape[0]:
            raise ValueError(f"the closed set holds token id {int(plan.edge_token.max())}, the output projection has {weight.shape[0]} rows")
        per = max(1, self.max_rows // bsz)
        for c0 in range(0, plan.C, per):
            c1 = min(plan.C, c0 + per)
            i0, i1, T = plan.chunk_items(c0, c1)
            if i1 == i0:                                      # only repeats of earlier answers: no new node
                continue
            n = c1 - c0
            # rows ordered (sentence, answer) as the reference: encoder rows repeat_interleave'd, answers tiled
            enc_c = model.encoder.reorder_encoder_out(enc, torch.arange(bsz, device=device).repeat_interleave(n))
            prev = dev["prev_output_tokens"][c0:c1, :T].repeat(bsz, 1)
            h, _ = model.decoder([Slot(ModalityType.TEXT, False, prev)], encoder_out=enc_c, features_only=True)
            h2d = h.reshape(bsz * n * T, h.shape[-1])
            if h2d.dtype != weight.dtype:
                h2d = h2d.to(weight.dtype)
            K.closed_set_edge_logits(h2d, weight, bias, dev, bsz, n, T, c0, dev["items"][i0:i1], buf["ws"])
        K.closed_set_reduce(dev, bsz, buf["ws"], buf["scores"])
        return buf["scores"].cpu()

    # ------------------------------------------------------------------ trie-constrained beam search (generator.TrieBeamGenerator)
    def trie_generator(self, **gen_kwargs):
        """The TrieBeamGenerator for these generator arguments (Task.generator_kwargs: `beam`, `return_n_best`, `max_len`,
        `normalize_scores` False by default, ...), kept so that its captured step graphs are reused by later batches."""
        from .generator import TrieBeamGenerator
        if self.plan is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) first")
        kw = self.generator_kwargs(**gen_kwargs)
        key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._trie_gens:
            self._trie_gens[key] = TrieBeamGenerator(self.global_dict, self.plan, **kw)
        return self._trie_gens[key]

    def _beam_hypotheses(self, model, sample, beam=None, n_best=1, **generator_options):
        model.eval()
        gen = self.trie_generator(beam=self.beam if beam is None else int(beam), return_n_best=int(n_best), **generator_options)
        return gen.generate(model, sample)

    def beam_search(self, model, sample, beam: Optional[int] = None, n_best: int = 1, **generator_options):
        """Beam search restricted to the answer trie: per sentence the best hypothesis (n_best = 1) or the list of the n_best best,
        as Task.inference returns them, `.text` filled through the text preprocessor.  Scores are unnormalised log-probabilities
        unless normalize_scores=True.  The model is left in eval mode."""
        outputs = self._beam_hypotheses(model, sample, beam, n_best, **generator_options)
        pre = self.general_preprocess.name2pre["text"]
        for single in outputs:
            for hyp in (single if isinstance(single, list) else [single]):
                hyp.text = pre.decode(hyp.tokens)
        return outputs

    def inference(self, model, sample, search: Optional[str] = None, **kwargs) -> List[object]:
        """The best answer of the closed set per sentence.  search "all" (the default of the constructor): every answer is scored,
        ties to the lower answer index.  search "beam": the answer spelled by the best hypothesis of `beam_search(**kwargs)`
        (duplicate answers: the lowest label) -- the reference's route, not necessarily the arg-max.  The model is left in eval
        mode."""
        search = self.search if search is None else search
        if search not in self.SEARCHES:
            raise ValueError(f"TraverseTask.inference: search must be one of {self.SEARCHES}, got {search!r}")
        if search == "beam":
            kwargs.pop("n_best", None)
            out = []
            # (the hypotheses are mapped by token sequence: no text decoding, which costs milliseconds per hypothesis on the host)
            for b, hyp in enumerate(self._beam_hypotheses(model, sample, n_best=1, **kwargs)):
                seq = tuple(hyp.tokens[:-1].tolist())
                if seq not in self._seq2label:
                    raise ValueError(f"task {self.name}: the hypothesis of sentence {b} ({list(seq)}) is not an answer of the closed set")
                out.append(self.index2ans[self._seq2label[seq]])
            return out
        scores = self.score(model, sample)
        best = np.argmax(scores.numpy(), axis=1)              # numpy: the first maximum
        return [self.index2ans[int(i)] for i in best]
