"""The state rules every optional per-run output follows ("The slot of an optional output"): a switch, an
engine-owned buffer that only grows, a caller-owned buffer that set_batch forgets, a record of where the last run put its result --
walked through once per kind of output on one long-lived engine.

Expected values: a fresh Engine per batch that does nothing but forward(); equality is bit-exact.  Parity against the oracle is the
job of tests/test_embeddings_gpu.py, test_node_embeddings_gpu.py, test_node_logits_gpu.py and test_attention_gpu.py.
Shapes: 6 and 48 molecules -- the smallest pair at which the second batch cannot fit the buffer sized for the first."""
import numpy as np
import pytest

from flowgnn_amd import Engine, FlowGNNError
from tests.test_embeddings_gpu import model_batch, model_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """As tests/test_embeddings_gpu.py: torch's HIP context before the first engine exists."""
    if torch.cuda.is_available():
        torch.cuda.init()


class Kind:
    """One kind of output: how to switch it on, read it (always as a tuple of arrays), find it and redirect it."""

    def __init__(self, name, forward_arg, getter, device_ptrs, set_buffers):
        self.name, self.forward_arg, self.getter, self.device_ptrs, self.set_buffers = name, forward_arg, getter, device_ptrs, set_buffers

    @staticmethod
    def _tuple(v):
        return tuple(v) if isinstance(v, tuple) else (v,)

    def switch_on(self, e, how=True):
        getattr(e, "set_" + self.name)(how)

    def get(self, e):
        return self._tuple(getattr(e, self.getter)())

    def ptrs(self, e):
        return self._tuple(getattr(e, self.device_ptrs)())

    def redirect(self, e, tensors):
        getattr(e, self.set_buffers)(*(t.data_ptr() for t in tensors))

    def fresh(self, model, w, b, how=True):
        e = Engine(model, device=0)
        try:
            e.set_weights(w)
            return self._tuple(e.forward(b, **{self.forward_arg: how})[1])
        finally:
            e.close()


KINDS = {
    "embeddings": Kind("embeddings", "return_embeddings", "embeddings", "embeddings_device_ptr", "set_embeddings_buffer"),
    "node_embeddings": Kind("node_embeddings", "return_node_embeddings", "node_embeddings", "node_embeddings_device_ptr",
                            "set_node_embeddings_buffer"),
    "node_logits": Kind("node_logits", "return_node_logits", "node_logits", "node_logits_device_ptr", "set_node_logits_buffer"),
    "attention": Kind("attention", "return_attention", "attention", "attention_device_ptrs", "set_attention_buffers"),
}


def same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def refuses(*fns):
    for fn in fns:
        with pytest.raises(FlowGNNError) as ei:
            fn()
        assert ei.value.code == 6, fn


@pytest.mark.parametrize("kind,model,how", [("embeddings", "GIN", True), ("node_embeddings", "GCN", True), ("node_logits", "GIN", True),
                                            ("attention", "GAT", "last")])
def test_slot_rules(kind, model, how):
    k = KINDS[kind]
    w = model_weights(model)
    small, big = model_batch(model, 6, seed=5), model_batch(model, 48, seed=6)
    want_small, want_big = k.fresh(model, w, small, how), k.fresh(model, w, big, how)
    assert all(b.size > s.size for s, b in zip(want_small, want_big))
    e = Engine(model, device=0)
    try:
        e.set_weights(w)
        k.switch_on(e, how)
        # 1. the small batch
        e.set_batch(small)
        e.run()
        assert same(k.get(e), want_small)
        # 2. a new batch: nothing to be had before its first run
        e.set_batch(big)
        refuses(lambda: k.get(e), lambda: k.ptrs(e))
        # 3. the engine's own buffer regrew
        e.run()
        assert same(k.get(e), want_big)
        grown = k.ptrs(e)
        assert all(grown)
        # 4. ... and only grows: the small batch again lands in the same allocation
        e.set_batch(small)
        e.run()
        assert same(k.get(e), want_small)
        assert k.ptrs(e) == grown
        # 5. a caller-owned buffer receives the same bits
        mine = [torch.zeros(a.shape, dtype=torch.float32, device="cuda:0") for a in want_small]
        torch.cuda.synchronize()
        k.redirect(e, mine)
        e.run()
        assert k.ptrs(e) == tuple(t.data_ptr() for t in mine)
        assert same(k.get(e), want_small)
        assert same(tuple(t.cpu().numpy() for t in mine), want_small)
        # 6. ... and set_batch forgets it
        for t in mine:
            t.zero_()
        torch.cuda.synchronize()
        e.set_batch(small)
        e.run()
        assert same(k.get(e), want_small)
        assert all(p != t.data_ptr() for p, t in zip(k.ptrs(e), mine)) and k.ptrs(e) == grown
        assert not any(t.cpu().numpy().any() for t in mine)
        # 7. a tap's pass leaves the run's outputs alone
        e.final_h()
        assert same(k.get(e), want_small)
        assert not any(t.cpu().numpy().any() for t in mine)
        # 8. attention: the mask is the switch of both buffers, and a mask changed since the run is "not the last run's"
        if kind == "attention":
            want_all = k.fresh(model, w, small, "all")
            e.set_attention("all")
            refuses(e.attention, e.attention_device_ptrs)
            e.run()
            assert same(k.get(e), want_all)
            e.set_attention("last")
            e.run()
            assert same(k.get(e), want_small)
    finally:
        e.close()
