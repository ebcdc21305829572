"""Generates tests/golden/ref_weights_<model>.npz: the TRAINED weight sets the reference ships as raw float32 .bin files
(GIN/*.bin, GCN/gcn_ep1_dim100.weights.all.bin, GAT/*.bin, PNA/pna_ep1_noBN_dim80.weights.all.bin, DGN/dgn_ep1_noBN_dim100.weights.all.bin;
GIN-VN ships the same files as GIN), read with this repo's loaders (flowgnn_amd/weights.py, which follow <M>/src/host_load.cc) and
stored tensor by tensor.  Data, not code: the GPU box has no /root/reference, and parity on trained weights (magnitudes the
synthetic sets do not have: GIN logits around -3 .. -6, PNA's saturating head) is otherwise only ever checked on the CPU.
The expected logits for them are the `logits_reference_weights` arrays of the per-model fixtures next to this file (oracle outputs).

A set larger than PART_BYTES is stored in parts (ref_weights_<model>.npz, ref_weights_<model>.1.npz, ...; a tensor larger than half a
part as its slices along the first axis, keys `<name>#<i>`) so that every committed file stays below 1 MiB; load() puts it together.

It also writes tests/golden/ref_files.json, the record of the shipped files themselves: size and SHA-256 of every file the saver
writes, and the 32-bit words in which the shipped file differs from what the saver writes from the loaded set (words no loader reads:
GCN's BatchNorm step counters, GIN's eps).  shipped_dir() rebuilds the files byte for byte from the fixture and that record, so the
tests read the reference's own weight files without a checkout of the reference.
Run from the repo root, with the reference checkout at $FLOWGNN_REFERENCE:  python tests/golden/make_ref_weights.py"""
import hashlib
import json
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flowgnn_amd import weights  # noqa: E402

REF = os.environ.get("FLOWGNN_REFERENCE", "/root/reference")
MODELS = ("GIN", "GCN", "GAT", "PNA", "DGN")
PART_BYTES = 900 * 1024  # raw float32 bytes per .npz part
RECORD = os.path.join(HERE, "ref_files.json")
MAX_PATCH_WORDS = 64     # more differing words than this: the saver does not reproduce the file, the record would be the file


def part_path(model, part):
    return os.path.join(HERE, f"ref_weights_{model.lower()}" + (f".{part}" if part else "") + ".npz")


def save(model, w):
    pieces = []
    for k, v in w.items():
        v = np.asarray(v, np.float32)
        pieces += [(f"{k}#{i}", v[i]) for i in range(v.shape[0])] if v.nbytes > PART_BYTES // 2 else [(k, v)]
    parts, size = [OrderedDict()], 0
    for k, v in pieces:
        if parts[-1] and size + v.nbytes > PART_BYTES:
            parts.append(OrderedDict())
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for i, p in enumerate(parts):
        np.savez_compressed(part_path(model, i), **p)
    return [part_path(model, i) for i in range(len(parts))]


def load(model):
    """The trained set of `model` (GIN-VN: GIN's) as the loader returns it from the shipped files."""
    model = "GIN" if model == "GIN-VN" else model
    flat, part = OrderedDict(), 0
    while os.path.exists(part_path(model, part)):
        z = np.load(part_path(model, part))
        flat.update((k, z[k]) for k in z.files)
        part += 1
    if not flat:
        raise FileNotFoundError(part_path(model, 0))
    w, sliced = OrderedDict(), {}
    for k, v in flat.items():
        name, sep, i = k.rpartition("#")
        if sep:
            w.setdefault(name, None)
            sliced.setdefault(name, {})[int(i)] = v
        else:
            w[k] = v
    for name, s in sliced.items():
        w[name] = np.stack([s[i] for i in range(len(s))])
    return w


def _words(path):
    return np.fromfile(path, dtype="<u4")


def record(model, ref_dir, tmp_dir):
    weights.SAVERS[model](load(model), tmp_dir)
    rec = OrderedDict()
    for f in sorted(os.listdir(tmp_dir)):
        shipped = os.path.join(ref_dir, f)
        data = open(shipped, "rb").read()
        ours, theirs = _words(os.path.join(tmp_dir, f)), _words(shipped)
        assert ours.shape == theirs.shape, (model, f, ours.shape, theirs.shape)
        diff = np.nonzero(ours != theirs)[0]
        assert len(diff) <= MAX_PATCH_WORDS, (model, f, len(diff))
        rec[f] = OrderedDict(bytes=len(data), sha256=hashlib.sha256(data).hexdigest(),
                             patch=[[int(i), int(theirs[i])] for i in diff])
    return rec


def shipped_dir(model, directory):
    """Rebuilds the reference's weight files of `model` (GIN-VN: GIN's) in `directory`, byte for byte: the fixture written by the saver,
    the recorded words patched in, every file checked against the recorded size and SHA-256.  Returns `directory`."""
    model = "GIN" if model == "GIN-VN" else model
    directory = str(directory)
    weights.SAVERS[model](load(model), directory)
    rec = json.load(open(RECORD))[model]
    assert sorted(rec) == sorted(os.listdir(directory)), (model, sorted(os.listdir(directory)))
    for f, r in rec.items():
        path = os.path.join(directory, f)
        if r["patch"]:
            a = _words(path)
            for i, bits in r["patch"]:
                a[i] = bits
            a.tofile(path)
        data = open(path, "rb").read()
        assert len(data) == r["bytes"] and hashlib.sha256(data).hexdigest() == r["sha256"], (model, f)
    return directory


if __name__ == "__main__":
    import tempfile
    for model in MODELS:
        for old in [part_path(model, i) for i in range(8)]:
            if os.path.exists(old):
                os.remove(old)
        w = weights.LOADERS[model](os.path.join(REF, model))
        paths = save(model, w)
        print(model, {k: v.shape for k, v in w.items()}, [os.path.getsize(p) for p in paths], "bytes")
    files = OrderedDict()
    for model in MODELS:
        with tempfile.TemporaryDirectory() as tmp:
            files[model] = record(model, os.path.join(REF, model), tmp)
    with open(RECORD, "w") as fh:
        json.dump(files, fh, indent=1)
        fh.write("\n")
    print("wrote", RECORD)
