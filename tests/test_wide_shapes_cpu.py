"""The width-300 family's shape sweeps and seeded random batches (tests/wide_cases.py), on the references alone:
what tests/test_wide_shapes_gpu.py relies on.  No GPU.

  1. Every (instance, case) pair the GPU file runs stays inside the fast path's range: operands(...) < 3e4, half the kernels' 6e4
     threshold.  (A shard of a random batch holds a subset of its graphs, and every operand is a maximum over rows or graphs that
     depend on their own graph alone: a shard's operands are at most the batch's.  The readout rows run the same layers.)
  2. The cases are what they claim: in-degrees, a source across a 128-row boundary, all 60 edge codes, N mod 128 and mod 16, and an
     edgeless graph, a self loop and a duplicate edge in the random set.
  3. The parity rule can see a one-row or a tail-column slip: with the residual's x_l, or the JK store, left out for the last node of
     the batch only, or for columns 288 .. 299 only, the reference's rows r miss 1e-4 (scale + |want|) by at least 10 x, on every
     fixed family of every default-mode instance that has the term.  (The f16 rows are not here: their rows are printed, not
     asserted, on the GPU.)
  4. The f16 reference differs from the fp64 one by less than the f16 rule allows on the logits, so the GPU's f16 comparison is not
     vacuous.

Caps (wide_cases.CAPS, RANDOM_MAX_NODES), chosen until 1. holds, and the maxima measured with them (printed by the tests):
  gcn          graphs <= 301 nodes (random: 129), up to 16 random edges per node, a 300-leaf hub:    operands <= 21, scale <= 80
  gcn-virtual  graphs <= 129 nodes, the same densities, a 100-leaf hub:                               operands <= 2.48e4 (sum, residual,
               isolated nodes), scale <= 7.7e3.  At 255 .. 257 nodes in one graph t alone passes 1e5: the tile-edge sizes above 129
               are laid out as 128-node graphs and a rest, which leaves every row where it was.
  gin          graphs <= 301 nodes (random: 33), <= 2.2 random edges per node, <= 3 duplicated edges, in-degree <= 6, a 40-leaf hub:
               operands <= 1.2e3 (the hub), scale <= 254
  gin-virtual  graphs <= 129 nodes (random: 33), otherwise as gin:                                    operands <= 1.86e4 (sum, residual,
               isolated nodes), scale <= 7.9e3; the f16 rows the same within a percent
  Smallest ratio of 3., printed per instance: gin 278 / 437 / 392 (last + residual / sum / sum + residual), gin-virtual 50.6 / 66.3 / 130,
  gcn 1 583 / 1 653 / 1 455, gcn-virtual 66.6 / 104 / 157; the smallest of all on family (c), the residual left out for the last node.
  Largest f16-against-fp64 ratio of 4.: 0.33 of the f16 rule (gin without the virtual node, where the scale is smallest).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import wide_cases as C  # noqa: E402
from tests.parity import err_ratio  # noqa: E402
from tests.test_gin_wide_f16_gpu import F16_REL  # noqa: E402

DEFAULT_WITH_A_TERM = [i for i in C.INSTANCES if not i.f16 and (i.res or i.jk == "sum")]
F16 = [i for i in C.INSTANCES if i.f16]
ids = lambda instances: [C.name_of(i) for i in instances]


# ---------------------------------------------------------------- 1. range
@pytest.mark.parametrize("instance", C.INSTANCES, ids=C.IDS)
def test_every_case_stays_in_range(instance):
    worst = (0.0, None)
    for name, b in C.cases_of(instance):
        ref = C.cached_reference(instance, name)
        if name == "f-256-nodes":
            assert ref.operands == C.operands(instance, b)  # (operands() is the reference's last field)
        print(C.name_of(instance), name, f"operands {ref.operands:.4g} scale {ref.scale:.4g} (N {b.total_nodes}, G {b.num_graphs})")
        assert np.isfinite(ref.rows).all() and np.isfinite(ref.logits).all()
        assert ref.operands < C.RANGE_LIMIT, (name, ref.operands)
        worst = max(worst, (ref.operands, name))
    print(C.name_of(instance), f"largest operand {worst[0]:.4g} ({worst[1]}) < {C.RANGE_LIMIT:g}")


def test_the_instance_table():
    assert len(C.INSTANCES) == 24 == len(set(C.INSTANCES)) and sum(i.f16 for i in C.INSTANCES) == 8
    assert all(i.kind == "gin" for i in C.INSTANCES if i.f16)
    assert {(i.kind, i.vn) for i in C.INSTANCES} == {(k, v) for k in ("gin", "gcn") for v in (False, True)}
    for i in C.INSTANCES:
        names = [n for n, _ in C.cases_of(i)]
        assert len(names) == (14 if i.vn else 9) and len(set(names)) == len(names), names


# ---------------------------------------------------------------- 2. the cases are what they claim
def indeg(b):
    return np.bincount(b.global_edges()[:, 1], minlength=b.total_nodes)


def codes(b):
    return (b.edge_attr[:, 0] * 6 + b.edge_attr[:, 1]) * 2 + b.edge_attr[:, 2]


@pytest.mark.parametrize("family", C.FAMILIES)
def test_the_fixed_cases_are_what_they_claim(family):
    caps, virtual = C.CAPS[family], family.endswith("-virtual")
    fixed = lambda name: C.fixed_batch(family, name)
    a, b, c = fixed("a-paths"), fixed("b-isolated"), fixed("c-gather")
    # (a), (b): every EDGE_COUNTS size ends where it ended -- the cumulative sums are boundaries between graphs -- and no graph passes the cap
    for x in (a, b):
        assert x.total_nodes == sum(C.EDGE_COUNTS) == 1489 and set(np.cumsum(C.EDGE_COUNTS)) <= set(x.node_offsets().tolist())
        assert x.nums_of_nodes.max() <= caps.max_nodes
    assert x.total_nodes % 128 == 81 and x.total_nodes % 16 == 1
    assert indeg(a).max() == 2 and b.total_edges == 0 and indeg(b).max() == 0
    assert set(C.EDGE_COUNTS) <= set(a.nums_of_nodes.tolist()) if not virtual else {n for n in C.EDGE_COUNTS if n <= 129} <= set(a.nums_of_nodes.tolist())
    ge = a.global_edges()
    assert (ge[:, 0] // 128 != ge[:, 1] // 128).any() and (ge[:, 0] // 16 != ge[:, 1] // 16).any()
    # (c): the hub's in-degree, all 60 edge codes, one-node graphs around it, a destination whose source lies across a 128-row boundary
    assert indeg(c).max() == caps.hub_leaves and len(np.unique(codes(c))) == 60
    assert (c.nums_of_nodes == 1).sum() == 4 and c.nums_of_nodes[0] == 1 and c.nums_of_nodes[-1] == 1
    ge = c.global_edges()
    assert (ge[:, 0] // 128 != ge[:, 1] // 128).any()
    assert c.nums_of_nodes.max() <= caps.max_nodes
    # (e): the graph counts around the update's 16-graph column tile
    if virtual:
        for G in C.GRAPH_COUNTS:
            e = fixed(f"e-{G}-graphs")
            assert e.num_graphs == G and 1 <= e.nums_of_nodes.min() and e.nums_of_nodes.max() <= 5
        assert [G % 16 for G in C.GRAPH_COUNTS] == [1, 15, 0, 1, 1]
    # (f): 128 k + 1, 128 k + 127, 128 k
    assert [fixed(f"f-{N}-nodes").total_nodes % 128 for N in (257, 383, 256)] == [1, 127, 0]
    assert [fixed(f"f-{N}-nodes").total_nodes % 16 for N in (257, 383, 256)] == [1, 15, 0]
    assert all(fixed(f"f-{N}-nodes").total_nodes == N for N in (257, 383, 256))


@pytest.mark.parametrize("family", C.FAMILIES)
def test_the_random_set_is_what_it_claims(family):
    caps = C.CAPS[family]
    batches = [C.random_case(s, family) for s in C.SEEDS]
    edgeless = loops = dups = 0
    seen_codes, sizes = set(), set()
    for s, b in zip(C.SEEDS, batches):
        again = C.random_batch(s, family)  # a pure function of its arguments
        assert all(np.array_equal(getattr(b, f), getattr(again, f)) for f in ("nums_of_nodes", "nums_of_edges", "node_feature", "edge_list", "edge_attr"))
        assert 1 <= b.num_graphs <= 39 and b.nums_of_nodes.max() <= C.RANDOM_MAX_NODES[family]
        assert 1 <= C.shard_cut(s, b) < b.num_graphs  # the shard check has two shards
        if caps.max_indeg is not None:
            assert indeg(b).max() <= caps.max_indeg
        edgeless += int((b.nums_of_edges == 0).sum())
        loops += int((b.edge_list[:, 0] == b.edge_list[:, 1]).sum())
        ge = b.global_edges()
        dups += len(ge) - len(np.unique(ge, axis=0))
        seen_codes |= set(codes(b).tolist())
        sizes |= set(b.nums_of_nodes.tolist())
        print(family, "seed", s, f"G {b.num_graphs} N {b.total_nodes} (mod 128: {b.total_nodes % 128}, mod 16: {b.total_nodes % 16}) E {b.total_edges} "
              f"largest in-degree {indeg(b).max()} largest graph {b.nums_of_nodes.max()}")
    assert edgeless >= 1 and loops >= 1 and dups >= 1, (edgeless, loops, dups)
    assert len(seen_codes) == 60
    assert 1 in sizes and max(sizes) >= 33, sizes  # tiny and larger graphs mixed
    assert len({b.total_nodes for b in batches}) == len(batches)


# ---------------------------------------------------------------- 3. a one-row or tail-column slip misses the rule by ten times
def masks(b):
    last, tail = np.zeros((b.total_nodes, 300), bool), np.zeros((b.total_nodes, 300), bool)
    last[-1, :] = True
    tail[:, 288:] = True
    return {"the last node": last, "columns 288..299": tail}


@pytest.mark.parametrize("instance", DEFAULT_WITH_A_TERM, ids=ids(DEFAULT_WITH_A_TERM))
def test_the_bound_sees_a_one_row_or_tail_column_slip(instance):
    terms = (["residual"] if instance.res else []) + (["jk"] if instance.jk == "sum" else [])
    smallest = (np.inf, None)
    for name, b in C.cases_of(instance):
        if name.startswith("random"):
            continue
        ref = C.cached_reference(instance, name)
        for term in terms:
            for where, mask in masks(b).items():
                wrong = C.reference(instance, b, drop=(term, mask))
                r = err_ratio(wrong.rows, ref.rows, ref.scale)
                if term == "jk":
                    assert np.array_equal(wrong.rows[~mask], ref.rows[~mask])  # (the JK sum is element-wise: the slip stays where it was made)
                print(C.name_of(instance), name, term, "dropped for", where, f"{r:.1f} x the rule")
                assert r >= 10.0, (name, term, where, r)
                smallest = min(smallest, (r, f"{name}, {term}, {where}"))
    print(C.name_of(instance), f"smallest ratio {smallest[0]:.1f} ({smallest[1]})")


# ---------------------------------------------------------------- 4. the f16 reference against the fp64 one
@pytest.mark.parametrize("instance", F16, ids=ids(F16))
def test_the_f16_reference_is_consistent_with_fp64(instance):
    plain = instance._replace(f16=False)
    for name, b in C.cases_of(instance):
        half, full = C.cached_reference(instance, name), C.cached_reference(plain, name)
        r = err_ratio(half.logits, full.logits, full.scale, F16_REL)
        print(C.name_of(instance), name, f"f16 reference against fp64, logits: {r:.4f} x the f16 rule (scale {full.scale:.4g})")
        assert not np.array_equal(half.logits, full.logits)
        assert r < 1.0, (name, r)
