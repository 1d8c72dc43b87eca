"""CPU: which micro-batch takes which criterion (ofasys_amd/criterion.py `route`).  A table of micro-batch dicts built from placeholder
values -- the route reads keys and scalars only -- crossed with the settings (edge head on / off, label_smoothing 0 or > 0,
constraint_range set or not, drop_worst_ratio 0 or > 0) and the direction (training / validation).  Each row names a route or a
refusal (type, fragment of the message: the fragments the GPU refusal tests match on); a mutation check keeps the table from going
vacuous."""
import itertools

import pytest
import torch

from ofasys_amd import criterion

X = torch.zeros(1)                              # presence is all that counts for a tensor-valued key
NODES = {"constraint_nodes": X, "constraint_trie": {"N": 1}}
STT = {"encoder_target": X, "ctc_range": "8,40"}

SETTINGS = [criterion.Settings(pad=1, eos=2, label_smoothing=ls, constraint_range=cr, drop_worst_ratio=dw, edge_head=head)
            for head, ls, cr, dw in itertools.product((False, True), (0.0, 0.1), (None, (4, 100)), (0.0, 0.25))]


def dense(cfg, training):
    return "label_smoothed" if cfg.label_smoothing > 0 or cfg.constraint_range is not None or cfg.drop_worst_ratio > 0 else "plain"


def closed(cfg, training):
    return "trie_head" if cfg.edge_head else "trie_nodes"


def always(what):
    return lambda cfg, training: what


def train_else(train, valid):
    return lambda cfg, training: train if training else valid


SCST_VALID = (NotImplementedError, "SCST")
NOT_BOTH = (ValueError, "not both")
NODES_REWARD = (NotImplementedError, "constraint_nodes")
NO_TRIE = (ValueError, "constraint_trie")
PACK_MASKS = (NotImplementedError, "pack plan")
REWARD_MASKS = (NotImplementedError, "constraint_masks")
STT_EXTRA = (NotImplementedError, "neither a reward nor constraint_nodes")
STT_WEIGHTS = (ValueError, "one of them must be positive")

# (name, the keys a micro-batch carries besides slots and target, expectation(settings, training))
TABLE = [
    ("bare", {}, dense),
    ("packed", {"pack": object()}, dense),
    ("task and scalars", {"task": "caption", "sentence_avg": True}, dense),
    ("masks", {"constraint_masks": X}, always("label_smoothed")),
    ("masks packed", {"constraint_masks": X, "pack": object()}, always(PACK_MASKS)),
    ("nodes", NODES, closed),
    ("nodes packed", dict(NODES, pack=object(), constraint_nodes_packed=X), closed),
    ("nodes and masks", dict(NODES, constraint_masks=X), always(NOT_BOTH)),
    ("nodes and masks packed: the pack refusal first", dict(NODES, constraint_masks=X, pack=object()), always(PACK_MASKS)),
    ("nodes and reward: the nodes' refusal, not SCST", dict(NODES, reward=X), train_else(NODES_REWARD, SCST_VALID)),
    ("nodes and reward without a trie: the reward first", {"constraint_nodes": X, "reward": X}, train_else(NODES_REWARD, SCST_VALID)),
    ("nodes without a trie", {"constraint_nodes": X}, always(NO_TRIE)),
    ("a trie without nodes", {"constraint_trie": {"N": 1}}, dense),
    ("reward", {"reward": X}, train_else("scst", SCST_VALID)),
    ("reward packed with its own range", {"reward": X, "pack": object(), "constraint_range": "4,100"}, train_else("scst", SCST_VALID)),
    ("reward and masks", {"reward": X, "constraint_masks": X}, train_else(REWARD_MASKS, SCST_VALID)),
    ("speech to text", STT, always("speech_to_text")),
    ("speech to text packed",dict(STT, pack=object(), ce_weight=0.5, ctc_weight=0.5), always("speech_to_text")),
    ("speech to text with masks", dict(STT, constraint_masks=X), always("speech_to_text")),
    ("encoder_target alone", {"encoder_target": X}, dense),
    ("ctc_range alone", {"ctc_range": "8,40"}, dense),
    ("speech to text, both weights zero", dict(STT, ce_weight=0.0, ctc_weight=0.0), train_else(STT_WEIGHTS, "speech_to_text")),
    ("speech to text, a negative weight", dict(STT, ce_weight=-1.0, ctc_weight=2.0), train_else(STT_WEIGHTS, "speech_to_text")),
    ("speech to text with a reward", dict(STT, reward=X), train_else(STT_EXTRA, SCST_VALID)),
    ("speech to text, bad weights and a reward: the weights first", dict(STT, reward=X, ce_weight=0.0), train_else(STT_WEIGHTS, SCST_VALID)),
    ("speech to text with nodes", dict(STT, **NODES), train_else(STT_EXTRA, "speech_to_text")),
    ("speech to text with nodes and a reward: the nodes' refusal", dict(STT, **NODES, reward=X), train_else(NODES_REWARD, SCST_VALID)),
]
KEYS = ("pack", "constraint_masks", "constraint_nodes", "constraint_trie", "reward", "encoder_target", "ctc_range")


def observe(extra, cfg, training):
    s = dict({"slots": [], "target": X}, **extra)
    try:
        return criterion.route(s, cfg, training)
    except (ValueError, NotImplementedError) as e:
        return type(e), str(e)


def agrees(got, want):
    if isinstance(want, str) or isinstance(got, str):
        return got == want
    return got[0] is want[0] and want[1] in got[1]


def mismatches(table):
    return [(name, cfg, training, got, expect(cfg, training))
            for name, extra, expect in table for cfg in SETTINGS for training in (True, False)
            for got in [observe(extra, cfg, training)] if not agrees(got, expect(cfg, training))]


def test_every_row_routes_as_the_table_says():
    bad = mismatches(TABLE)
    assert not bad, bad[:5]
    seen = {expect(cfg, t) for _, _, expect in TABLE for cfg in SETTINGS for t in (True, False)}
    assert set(criterion.ROUTES) <= seen                                       # every route is reached ...
    assert {SCST_VALID, NOT_BOTH, NODES_REWARD, NO_TRIE, PACK_MASKS, REWARD_MASKS, STT_EXTRA, STT_WEIGHTS} <= seen    # ... and every refusal


@pytest.mark.parametrize("name,extra,fragment", [
    ("nodes and masks", dict(NODES, constraint_masks=X), "not both"),
    ("nodes and reward", dict(NODES, reward=X), "constraint_nodes"),
    ("nodes without a trie", {"constraint_nodes": X}, "constraint_trie"),
    ("masks packed", {"constraint_masks": X, "pack": object()}, "pack plan"),
    ("reward and masks", {"reward": X, "constraint_masks": X}, "constraint_masks")], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_carry_the_fragments_the_gpu_tests_match(name, extra, fragment):
    """pytest.raises(match=) exactly as tests/test_closed_set_train_gpu.py, test_closed_set_head_gpu.py, test_scst_gpu.py and
    test_validation_gpu.py write it, with no model and no device."""
    kind = ValueError if fragment in ("not both", "constraint_trie") else NotImplementedError
    for cfg in SETTINGS:
        with pytest.raises(kind, match=fragment):
            criterion.route(dict({"slots": [], "target": X}, **extra), cfg)
    with pytest.raises(NotImplementedError, match="SCST"):
        criterion.route({"slots": [], "target": X, "reward": X}, SETTINGS[0], training=False)


def test_the_four_ways_a_plain_batch_becomes_label_smoothed():
    base = criterion.Settings(pad=1, eos=2)
    s = {"slots": [], "target": X}
    assert criterion.route(s, base) == "plain" == criterion.route(s, base, training=False)
    assert criterion.route(s, base._replace(label_smoothing=0.1)) == "label_smoothed"
    assert criterion.route(s, base._replace(constraint_range=(4, 100))) == "label_smoothed"
    assert criterion.route(s, base._replace(drop_worst_ratio=0.25)) == "label_smoothed"
    assert criterion.route(dict(s, constraint_masks=X), base) == "label_smoothed"
    assert criterion.route(s, base._replace(edge_head=True)) == "plain"        # (the head switch alone moves no caption batch)


@pytest.mark.parametrize("key", KEYS)
def test_an_absent_key_and_a_key_set_to_none_route_alike(key):
    """On every row of the table that does not carry the key: adding it as None changes nothing."""
    rows = [(n, e) for n, e, _ in TABLE if key not in e]
    assert len(rows) >= 5
    for name, extra in rows:
        for cfg in SETTINGS[::5]:
            for training in (True, False):
                got, same = observe(extra, cfg, training), observe(dict(extra, **{key: None}), cfg, training)
                assert got == same, (name, key, got, same)


def test_a_malformed_node_batch_under_the_edge_head_meets_the_dense_refusal():
    head = criterion.Settings(pad=1, eos=2, label_smoothing=0.1, edge_head=True)
    assert criterion.route(dict(NODES, slots=[], target=X), head) == "trie_head"
    for extra, want in ((dict(NODES, constraint_masks=X), NOT_BOTH), (dict(NODES, reward=X), NODES_REWARD), ({"constraint_nodes": X}, NO_TRIE)):
        assert agrees(observe(extra, head, True), want)
        assert agrees(observe(extra, head._replace(edge_head=False), True), want)


def test_the_table_is_not_vacuous():
    """Mutations of the EXPECTATION (the route under test untouched): two arms' order swapped -- nodes looked at before speech-to-text,
    reward before nodes, the head switch ignored, validation forgetting its reward refusal -- must each make the comparison fail."""
    def swapped(table, a, b):
        by = {n: (e, x) for n, e, x in table}
        return [(n, e, by[b][1] if n == a else by[a][1] if n == b else x) for n, e, x in table]
    assert mismatches(swapped(TABLE, "speech to text with nodes", "nodes"))
    assert mismatches(swapped(TABLE, "nodes and reward: the nodes' refusal, not SCST", "reward"))
    assert mismatches(swapped(TABLE, "masks", "bare"))
    assert mismatches([(n, e, (lambda cfg, t: "trie_nodes") if x is closed else x) for n, e, x in TABLE])
    assert mismatches([(n, e, (lambda cfg, t, x=x: x(cfg, True))) for n, e, x in TABLE])
    assert not mismatches(swapped(TABLE, "bare", "packed"))                    # (a swap of two equal arms is no mutation)
