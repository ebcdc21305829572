"""The engine's configuration calls, recorded (tests/golden/config_calls.json) and replayed (tests/test_config_calls_gpu.py).

A script names a model and a sequence of raw ctypes calls on ONE fresh engine.  `run` executes it and returns, per call,
(rc, flowgnn_last_error's text, state); the state is what the header's getters say: flowgnn_emb_dim, flowgnn_num_tasks,
flowgnn_pooling, flowgnn_gin_eps (its return value and the five values), flowgnn_ogb_virtual_node, flowgnn_gcn_virtual_node,
flowgnn_attention_pooling, flowgnn_set2set_pooling and flowgnn_jk_residual (its return value and the two settings).  No script sets
weights or a batch or calls flowgnn_run: no model kernel is launched.

flowgnn_last_error answers with the calling thread's text while the engine has none of its own, which is whatever an earlier engine of
the process left there; so `run` opens every script with one refused call (PRIME) that gives the engine a text of its own, and records
it as the script's entry 0.

    python -m tests.config_calls --record     # writes the fixture.  It was recorded ONCE, on the MI355X, from the engine.hip that
                                              # preceded engine_config.hip; a comparison that fails means the code is wrong, not the fixture.

The fixture holds each distinct text and each distinct state once; a script's entries are [rc, text index, state index]."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "config_calls.json")

MODELS = ("GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN")
F32, Q6_10, F16 = 0, 1, 2
MEAN, SUM, MAX = 0, 1, 2
MODES = (-1, 0, 1, 2, 3)
PRIME = ("flowgnn_set_pooling", -1)
NUM_MODE, NUM_DIM, NUM_MODEL_DIM, NUM_MODEL = ("flowgnn_set_numeric_mode", "flowgnn_set_numeric_mode_dim", "flowgnn_set_model_numeric_mode_dim",
                                               "flowgnn_set_model_numeric_mode")
WIDTH_CALLS = ("flowgnn_set_emb_dim", "flowgnn_set_model_emb_dim")
JK_CALLS = ("flowgnn_set_jk_residual", "flowgnn_set_model_jk_residual")
VN_CALLS = {"GIN": ("flowgnn_set_ogb_virtual_node", "flowgnn_set_ogb_virtual_node_dim"),
            "GCN": ("flowgnn_set_gcn_virtual_node", "flowgnn_set_gcn_virtual_node_dim")}
ATTN, S2S = "flowgnn_set_attention_pooling", "flowgnn_set_set2set_pooling"


# ---------------------------------------------------------------- tensors: ("t", count, fill, index or None, value) -> np.full, one element replaced
def tensor(count, fill=0.01, at=None, value=None):
    return ("t", int(count), float(fill), at, value)


def vn_counts(d):
    return (d, 4 * 2 * d * d, 4 * 2 * d, 4 * d * 2 * d, 4 * d)


def attn_counts(d):
    return (2 * d * d, 2 * d, 2 * d)


def s2s_counts(d, tasks=1):
    return (4 * d * 2 * d, 4 * d * d, 4 * d, 4 * d, tasks * 2 * d, tasks)


def fills(counts):
    return [tensor(n, 0.01 * (i + 1)) for i, n in enumerate(counts)]


def null_patterns(ts):
    """exactly one tensor NULL, for each tensor; then exactly one tensor non-NULL, for each tensor"""
    n = len(ts)
    return [[None if j == i else ts[j] for j in range(n)] for i in range(n)] + [[ts[j] if j == i else None for j in range(n)] for i in range(n)]


def non_finite(ts):
    """NaN and +inf at the first and at the last element of each tensor"""
    out = []
    for i, t in enumerate(ts):
        for value in ("nan", "inf"):
            for at in (0, t[1] - 1):
                out.append([tensor(t[1], t[2], at, value) if j == i else ts[j] for j in range(len(ts))])
    return out


# ---------------------------------------------------------------- the scripts
def widen(model):
    return [("flowgnn_set_emb_dim", 300)] if model == "GIN" else [("flowgnn_set_model_emb_dim", 300)]


def reachable():
    """(name, model, calls that lead there): each model at its default width, GIN and GCN at 300"""
    return [(m.lower(), m, []) for m in MODELS] + [("gin-300", "GIN", [("flowgnn_set_emb_dim", 300)]), ("gcn-300", "GCN", [("flowgnn_set_model_emb_dim", 300)])]


def numeric_calls(modes=MODES):
    calls = [(NUM_MODE, m) for m in modes]
    for fn in (NUM_DIM, NUM_MODEL_DIM):
        calls += [(fn, d, m) for d in (80, 100, 200, 300) for m in modes]
    calls += [(NUM_MODEL, mid, m) for mid in range(-1, 7) for m in modes]
    return calls


def q6_10_through_all_four(model, widths=(100,)):
    calls = [(NUM_MODE, Q6_10)]
    for d in widths:
        calls += [(NUM_DIM, d, Q6_10), (NUM_MODEL_DIM, d, Q6_10)]
    return calls + [(NUM_MODEL, MODELS.index(model), Q6_10)]


def scripts():
    out = []

    def add(name, model, calls):
        out.append({"name": name, "model": model, "calls": list(calls)})

    # ---- numeric mode: every call on every reachable state, each followed by the plain reset
    for name, model, lead in reachable():
        calls = list(lead)
        for c in numeric_calls():
            calls += [c, (NUM_MODE, F32)]
        add("numeric/" + name, model, calls)
    # ... and Q6_10 through all four calls against each state that blocks it
    vn100 = fills(vn_counts(100))
    blockers = [("sum-pooling", "GIN", [("flowgnn_set_pooling", SUM)]), ("max-pooling", "GCN", [("flowgnn_set_pooling", MAX)]),
                ("eps", "GIN", [("flowgnn_set_gin_eps", ("eps", (0.25, 0.0, -0.5, 1.0, 2.0)))]),
                ("ogb-vn", "GIN", [(VN_CALLS["GIN"][0], *vn100)]), ("gcn-vn", "GCN", [(VN_CALLS["GCN"][0], *vn100)]),
                ("embeddings", "GIN", [("flowgnn_set_embeddings", 1)]), ("node-embeddings", "GCN", [("flowgnn_set_node_embeddings", 1)]),
                ("node-logits", "GIN", [("flowgnn_set_node_logits", 1)]), ("attention", "GAT", [("flowgnn_set_attention", 5)]),
                ("pna-embeddings", "PNA", [("flowgnn_set_embeddings", 1)]), ("dgn-node-embeddings", "DGN", [("flowgnn_set_node_embeddings", 1)]),
                ("two-tasks", "GIN", [("flowgnn_set_num_tasks", 2)])]
    for name, model, lead in blockers:
        add("numeric-q6_10/" + name, model, lead + q6_10_through_all_four(model, (80, 100) if model == "PNA" else (100,)))

    # ---- width
    for model in MODELS:
        add("width/" + model.lower(), model, [(fn, d) for fn in WIDTH_CALLS for d in (0, 100, 200, 300)] + [(fn, 100) for fn in WIDTH_CALLS])
    both_ways = [(fn, d) for fn in WIDTH_CALLS for d in (300, 100)]
    for model in ("GIN", "GCN"):
        vn, vn_dim = VN_CALLS[model]
        f16_at_300 = (NUM_DIM if model == "GIN" else NUM_MODEL_DIM, 300, F16)
        off = [None] * 5
        calls = [(NUM_MODE, F16)] + both_ways + [(NUM_MODE, Q6_10)] + both_ways + [(NUM_MODE, F32)]
        calls += widen(model) + [f16_at_300] + both_ways + [(NUM_MODE, F32)] + both_ways
        add("width-blocked/%s/numeric" % model.lower(), model, calls)
        calls = [(vn, *vn100)] + both_ways + [(vn, *off)] + widen(model) + [(vn_dim, 300, *fills(vn_counts(300)))] + both_ways + [(vn_dim, 300, *off)] + both_ways
        add("width-blocked/%s/virtual-node" % model.lower(), model, calls)
        readouts = [("attention-pooling", (ATTN, 300, *fills(attn_counts(300))), (ATTN, 300, None, None, None)),
                    ("set2set", (S2S, 300, 2, 1, *fills(s2s_counts(300))), (S2S, 300, 0, 0, *[None] * 6)),
                    ("jk-sum", (JK_CALLS[1], 300, 1, 0), (JK_CALLS[1], 300, 0, 0)), ("residual", (JK_CALLS[1], 300, 0, 1), (JK_CALLS[1], 100, 0, 0))]
        for name, on, turn_off in readouts:
            add("width-blocked/%s/%s" % (model.lower(), name), model, [on] + both_ways + widen(model) + [on] + both_ways + [turn_off] + both_ways)

    # ---- the virtual-node calls
    for model in ("GIN", "GCN"):
        vn, vn_dim = VN_CALLS[model]
        vn300 = fills(vn_counts(300))
        off = [None] * 5
        calls = [(vn_dim, d, *t) for d in (0, 200) for t in (off, vn100)]
        for p in null_patterns(vn100):
            calls += [(vn, *p), (vn_dim, 100, *p)]
        calls += [(vn_dim, 100, *p) for p in non_finite(vn100)] + [(vn, *p) for p in non_finite(vn100)[::5]]
        calls += [(vn_dim, 300, *vn300), (vn_dim, 300, *off)]  # tensors wider than the engine
        calls += [(NUM_MODE, Q6_10), (vn, *vn100), (vn_dim, 100, *vn100), (vn, *off), (NUM_MODE, F32)]
        calls += [(vn, *vn100), (vn_dim, 300, *off), (vn_dim, 100, *vn100), (vn, *off), (vn_dim, 100, *vn100), (vn_dim, 100, *off)]
        calls += widen(model)
        calls += [(vn, *vn100), (vn, *off), (vn_dim, 100, *vn100), (vn_dim, 100, *off)]  # tensors narrower than the engine
        calls += [(vn_dim, 300, *p) for p in null_patterns(vn300)[::3]] + [(vn_dim, 300, *p) for p in non_finite(vn300)[::3]]
        calls += [(vn_dim, 300, *vn300), (vn_dim, 100, *off), (vn_dim, 300, *vn300), (vn, *off), (vn_dim, 300, *vn300), (vn_dim, 300, *off)]
        add("virtual-node/" + model.lower(), model, calls)
    for model in MODELS:  # the wrong model: each engine hears all four calls
        calls = []
        for m in ("GIN", "GCN"):
            if m != model:
                vn, vn_dim = VN_CALLS[m]
                calls += [(vn, *[None] * 5), (vn, *vn100), (vn_dim, 100, *[None] * 5), (vn_dim, 100, *vn100), (vn_dim, 200, *vn100), (vn_dim, 300, *[None] * 5)]
        add("virtual-node-wrong-model/" + model.lower(), model, calls)

    # ---- the two readouts
    a100, a300 = fills(attn_counts(100)), fills(attn_counts(300))
    s100, s300 = fills(s2s_counts(100)), fills(s2s_counts(300))
    a_off, s_off = [None] * 3, [None] * 6
    for model in ("GIN", "GCN"):
        calls = [(ATTN, d, *t) for d in (0, 200) for t in (a_off, a300)]
        calls += [(ATTN, 300, *a300), (ATTN, 100, *a100), (ATTN, 100, *a_off), (ATTN, 300, *a_off)]  # an engine at width 100
        calls += [(NUM_MODE, Q6_10), (ATTN, 100, *a100), (ATTN, 300, *a300), (NUM_MODE, F32)]
        calls += widen(model)
        calls += [(ATTN, 100, *a100)]
        calls += [(ATTN, 300, *p) for p in null_patterns(a300)] + [(ATTN, 300, *p) for p in non_finite(a300)]
        calls += [("flowgnn_set_pooling", SUM), (ATTN, 300, *a300), ("flowgnn_set_pooling", MAX), (ATTN, 300, *a300), ("flowgnn_set_pooling", MEAN)]
        calls += [("flowgnn_set_node_logits", 1), (ATTN, 300, *a300), ("flowgnn_set_node_logits", 0)]
        calls += [(S2S, 300, 2, 1, *s300), (ATTN, 300, *a300), (S2S, 300, 2, 1, *s_off)]
        calls += [(ATTN, 300, *a300), (S2S, 300, 2, 1, *s300), ("flowgnn_set_pooling", SUM), ("flowgnn_set_pooling", MEAN), ("flowgnn_set_node_logits", 1)]
        calls += [(ATTN, 300, *a300), (ATTN, 100, *a_off), (ATTN, 300, *a300), (ATTN, 300, *a_off)]
        add("attention-pooling/" + model.lower(), model, calls)

        calls = [(S2S, d, 2, 1, *t) for d in (0, 200) for t in (s_off, s300)]
        calls += [(S2S, 300, 2, 1, *s300), (S2S, 100, 2, 1, *s100), (S2S, 100, 2, 1, *s_off), (S2S, 300, 0, 0, *s_off)]  # an engine at width 100
        calls += [(NUM_MODE, Q6_10), (S2S, 100, 2, 1, *s100), (S2S, 300, 2, 1, *s300), (NUM_MODE, F32)]
        calls += widen(model)
        calls += [(S2S, 100, 2, 1, *s100)]
        calls += [(S2S, 300, 2, 1, *p) for p in null_patterns(s300)] + [(S2S, 300, 2, 1, *p) for p in non_finite(s300)]
        for steps in (0, 1, 8, 9):
            calls += [(S2S, 300, steps, 1, *s300), (S2S, 300, steps, 1, *s_off)]
        calls += [(S2S, 300, 2, t, *fills(s2s_counts(300, max(t, 1)))) for t in (0, 2)]  # a num_tasks that is not the engine's
        calls += [("flowgnn_set_num_tasks", 3), (S2S, 300, 2, 1, *s300), (S2S, 300, 2, 3, *fills(s2s_counts(300, 3))), ("flowgnn_set_num_tasks", 2),
                  ("flowgnn_set_num_tasks", 3), ("flowgnn_set_num_tasks", 0), (S2S, 300, 2, 3, *s_off), ("flowgnn_set_num_tasks", 1)]
        calls += [("flowgnn_set_pooling", SUM), (S2S, 300, 2, 1, *s300), ("flowgnn_set_pooling", MAX), (S2S, 300, 2, 1, *s300), ("flowgnn_set_pooling", MEAN)]
        calls += [("flowgnn_set_node_logits", 1), (S2S, 300, 2, 1, *s300), ("flowgnn_set_node_logits", 0)]
        calls += [("flowgnn_set_embeddings", 1), (S2S, 300, 2, 1, *s300), ("flowgnn_set_embeddings", 0)]
        calls += [(S2S, 300, 2, 1, *s300), ("flowgnn_set_pooling", MAX), ("flowgnn_set_pooling", MEAN), ("flowgnn_set_node_logits", 1), ("flowgnn_set_embeddings", 1)]
        calls += [(S2S, 300, 8, 1, *s300), (S2S, 100, 0, 0, *s_off), (S2S, 300, 1, 1, *s300), (S2S, 300, 2, 1, *s_off)]
        add("set2set/" + model.lower(), model, calls)
    for model in ("GIN-VN", "GAT", "PNA", "DGN"):  # the wrong model
        add("readouts-wrong-model/" + model.lower(), model,
            [(ATTN, 300, *a300), (ATTN, 100, *a100), (ATTN, 300, *a_off), (ATTN, 200, *a_off), (S2S, 300, 2, 1, *s300), (S2S, 100, 2, 1, *s100),
             (S2S, 300, 2, 1, *s_off), (S2S, 200, 2, 1, *s_off), (S2S, 300, 0, 1, *s300), (S2S, 300, 2, 2, *s300)])

    # ---- JK / residual: both calls on every reachable state
    for name, model, lead in reachable():
        calls = list(lead) + [(fn, d, jk, res) for fn in JK_CALLS for d in (0, 100, 300) for jk in (-1, 0, 1, 2) for res in (-1, 0, 1, 2)]
        add("jk-residual/" + name, model, calls + [(JK_CALLS[0], 100, 0, 0)])

    # ---- the rest
    for model in MODELS:
        calls = [("flowgnn_set_num_tasks", t) for t in (0, 2, 1)]
        calls += [("flowgnn_set_pooling", m) for m in (-1, 3, SUM, MAX, MEAN)]
        calls += [(NUM_MODE, Q6_10), ("flowgnn_set_pooling", SUM), ("flowgnn_set_pooling", MEAN), (NUM_MODE, F32)]
        calls += [("flowgnn_set_node_logits", 1), ("flowgnn_set_pooling", MAX), ("flowgnn_set_pooling", MEAN), ("flowgnn_set_node_logits", 0)]
        good = (0.25, 0.0, -0.5, 1.0, 2.0)
        calls += [("flowgnn_set_gin_eps", ("eps", tuple(v if j == i else 0.5 for j in range(5)))) for i in (0, 4) for v in ("nan", "inf", "-inf")]
        calls += [("flowgnn_set_gin_eps", ("eps", good)), ("flowgnn_set_gin_eps", None), (NUM_MODE, Q6_10), ("flowgnn_set_gin_eps", ("eps", good)),
                  ("flowgnn_set_gin_eps", ("eps", ("nan",) * 5)), ("flowgnn_set_gin_eps", None), (NUM_MODE, F32), ("flowgnn_set_gin_eps", ("eps", good))]
        add("rest/" + model.lower(), model, calls)
    assert len({s["name"] for s in out}) == len(out)
    return out


# ---------------------------------------------------------------- the runner
_arrays = {}


def _array(spec):
    if spec not in _arrays:
        if spec[0] == "eps":
            a = np.array([float(v) for v in spec[1]], np.float32)
        else:
            _, count, fill, at, value = spec
            a = np.full(count, fill, np.float32)
            if at is not None:
                a[at] = float(value)
        _arrays[spec] = a
    return _arrays[spec]


def _arg(a):
    if a is None or isinstance(a, int):
        return a
    return _array(a).ctypes.data_as(C.POINTER(C.c_float))


def state(lib, h):
    eps = (C.c_float * 5)()
    jk, res = C.c_int(-7), C.c_int(-7)
    eps_on = lib.flowgnn_gin_eps(h, eps)
    jk_on = lib.flowgnn_jk_residual(h, C.byref(jk), C.byref(res))
    return [lib.flowgnn_emb_dim(h), lib.flowgnn_num_tasks(h), lib.flowgnn_pooling(h), eps_on, [float(v) for v in eps], lib.flowgnn_ogb_virtual_node(h),
            lib.flowgnn_gcn_virtual_node(h), lib.flowgnn_attention_pooling(h), lib.flowgnn_set2set_pooling(h), jk_on, jk.value, res.value]


def run(script):
    """[(rc, text, state)] of PRIME and then of every call of the script, on one fresh engine"""
    from flowgnn_amd import Engine
    e = Engine(script["model"])
    try:
        out = []
        for fn, *args in [PRIME] + script["calls"]:
            rc = getattr(e.lib, fn)(e._h, *[_arg(a) for a in args])
            text = (e.lib.flowgnn_last_error(e._h) or b"").decode("latin-1")
            out.append((rc, text, state(e.lib, e._h)))
        return out
    finally:
        e.close()


# ---------------------------------------------------------------- the fixture
def load_fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    return {name: [(rc, d["texts"][t], d["states"][s]) for rc, t, s in entries] for name, entries in d["scripts"].items()}


def record():
    texts, states, recorded = {}, {}, {}
    for s in scripts():
        recorded[s["name"]] = [[rc, texts.setdefault(text, len(texts)), states.setdefault(json.dumps(st), len(states))] for rc, text, st in run(s)]
    flat = lambda x: json.dumps(x, separators=(",", ":"))
    lines = ['{"texts": [\n' + ",\n".join(flat(t) for t in texts) + "\n],", '"states": [\n' + ",\n".join(flat(json.loads(s)) for s in states) + "\n],",
             '"scripts": {\n' + ",\n".join(flat(name) + ": " + flat(entries) for name, entries in recorded.items()) + "\n}}"]
    with open(FIXTURE, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%s: %d scripts, %d calls, %d texts, %d states" % (FIXTURE, len(recorded), sum(len(v) for v in recorded.values()), len(texts), len(states)))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.config_calls --record")
    record()
