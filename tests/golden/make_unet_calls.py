"""Writes tests/golden/unet_calls.json: every library call the UNet dispatch (free-hunch_amd/unet_hip.py) makes for a
forward pass and its input-VJP, in order, for five small configurations.  No device is needed: the passes run on CPU
tensors with `_lib.load` replaced by a recording proxy and `_lib.stream` by `lambda: None`, so no kernel executes.  The
committed file was written by the dispatch and the library as they stood before the convolution and GroupNorm routes were
folded into one path each; tests/test_unet_calls.py holds every later state to it, row for row.

The proxy forwards the host-only queries (QUERIES) to the built library and keeps each distinct (name, args) -> answer in
a table of its own; every other call is a launch: it is appended to the trace and answered with 0.  The queries are also
kept in the trace, so their order against the launches is part of the record.  Per argument a row holds null, the
integer / float value, or for a device pointer the token "pK" - K the position (struct fields counted in place) of the
first argument of the SAME call with that address, which is how the in-place cases show (dx being acc_src).  Where the
address is the start of a tensor that unet_hip allocated (torch.empty / zeros / empty_like, noted by a shim of the name
`torch` inside unet_hip that also keeps those tensors alive so that no address comes back) the token carries its size in
bytes, "pK:bytes": a workspace or partials buffer of the wrong size shows here.  Addresses themselves, and offsets between
tensors, are not recorded (the interior offsets of the three-kernel attention stay with its GPU test).  A by-reference
struct (fh_gn_epilogue) is a nested list of its fields.

    python tests/golden/make_unet_calls.py [--root CHECKOUT] [--out FILE] [--commit NAME]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

QUERIES = ("fh_conv2d_splitk", "fh_conv2d_x6_gn_chunks", "fh_conv2d_x6_norm_supported", "fh_groupnorm_small_supported",
           "fh_groupnorm_scratch_doubles", "fh_attention_supported", "fh_unet_set_precision", "fh_unet_get_precision")

_A = (256, 128, 1, (1, 1, 2, 2), True, "8", 4, 64, True, True, False)
_B = (32, 32, 1, (1, 2), True, "2", 4, 16, False, False, False)
# name -> (UNetConfig positional arguments, batch, UNetModel dtype, unet_hip.CONV_MODE)
TRACES = {"A": (_A, 1, "fp32", "x6"), "A4": (_A, 1, "fp16x3", "x6"), "B": (_B, 2, "fp32", "x6"),
          "Aw": (_A, 1, "fp32", "wino"), "Af": (_A, 1, "fp32", "f32")}


class _Recorder:
    """stands in for the loaded library: answers the queries through the real one, lists everything else"""

    def __init__(self, real):
        self.real, self.queries, self.calls, self.sizes, self.keep = real, {}, [], {}, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in QUERIES:
            def call(*args):
                answer = fn(*args)
                self.queries.setdefault((name, args), answer)
                self.calls.append(["?" + name, list(args), answer])
                return answer
        else:
            types = fn.argtypes

            def call(*args):
                assert len(args) == len(types), (name, len(args), len(types))
                self.calls.append([name] + self._encode(types, args))
                return 0
        self.__dict__[name] = call
        return call

    def _encode(self, types, args):
        first, pos = {}, [0]

        def one(tp, v):
            k = pos[0]
            pos[0] += 1
            if tp is C.c_void_p:  # a device pointer (or the stream)
                if not v:
                    return None
                size = self.sizes.get(v)
                tok = "p%d" % first.setdefault(v, k)
                return tok if size is None else "%s:%d" % (tok, size)
            if v is None:
                return None
            return float(v) if tp in (C.c_float, C.c_double) else int(v)

        row = []
        for tp, v in zip(types, args):
            if isinstance(getattr(tp, "_type_", None), type) and issubclass(tp._type_, C.Structure):  # passed with byref
                if v is None:
                    row.append(one(C.c_void_p, None))
                else:
                    s = v._obj
                    row.append([one(ft, getattr(s, fn)) for fn, ft in type(s)._fields_])
            else:
                row.append(one(tp, v))
        return row


class _TorchShim:
    """the name `torch` inside unet_hip: everything is torch's, but the allocations are noted (address -> bytes) and kept"""

    def __init__(self, torch, rec):
        self._torch, self._rec = torch, rec
        for name in ("empty", "zeros", "empty_like"):
            setattr(self, name, self._noting(getattr(torch, name)))

    def _noting(self, fn):
        def alloc(*a, **k):
            t = fn(*a, **k)
            if t.numel():
                self._rec.sizes[t.data_ptr()] = t.numel() * t.element_size()
                self._rec.keep.append(t)
            return t
        return alloc

    def __getattr__(self, name):
        return getattr(self._torch, name)


def record(unet, unet_hip, _lib, patch, names=None):
    """-> (query table {(name, args): answer}, {trace name: [row, ...]}) of the current code.  `patch(obj, name, value)`
    sets an attribute for the duration (pytest's monkeypatch.setattr, or `patched()` below)."""
    import torch
    real = _lib.load()
    queries, traces = {}, {}
    for name in names or TRACES:
        cfg_args, n, dtype, conv_mode = TRACES[name]
        rec = _Recorder(real)
        patch(_lib, "load", lambda rec=rec: rec)
        patch(_lib, "stream", lambda: None)
        patch(unet_hip, "CONV_MODE", conv_mode)
        patch(unet_hip, "torch", _TorchShim(torch, rec))
        cfg = unet.UNetConfig(*cfg_args)
        model = unet.UNetModel(cfg, dtype=dtype)
        model.load_state_dict(unet.seeded_state(cfg, 0))
        x = torch.zeros(n, cfg.in_channels, cfg.image_size, cfg.image_size, requires_grad=True)
        y = model(x, torch.full((n,), 3))
        torch.autograd.grad(y, x, torch.ones_like(y))
        for key, answer in rec.queries.items():
            assert queries.setdefault(key, answer) == answer, key
        traces[name] = rec.calls
        rec.keep.clear()  # (the trace has ended; `patch` may hold the recorder itself for longer)
    return queries, traces


def pack(queries, traces, about):
    """the fixture's layout: the table of distinct rows, and per trace the indices into it"""
    index, rows, packed = {}, [], {}
    for name, calls in traces.items():
        ids = []
        for row in calls:
            key = json.dumps(row)
            if key not in index:
                index[key] = len(rows)
                rows.append(row)
            ids.append(index[key])
        packed[name] = ids
    return {"about": about,
            "configs": {k: {"config": list(v[0]), "N": v[1], "dtype": v[2], "CONV_MODE": v[3]} for k, v in TRACES.items()},
            "queries": sorted([n, list(a), r] for (n, a), r in queries.items()), "rows": rows, "traces": packed}


def unpack(doc):
    """-> (query table, traces) in the form `record` returns (through JSON: tuples are lists)"""
    queries = {(n, tuple(a)): r for n, a, r in doc["queries"]}
    return queries, {name: [doc["rows"][i] for i in ids] for name, ids in doc["traces"].items()}


class patched:
    """setattr with the old values put back on exit"""

    def __init__(self):
        self.undo = []

    def __call__(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for obj, name, old in reversed(self.undo):
            setattr(obj, name, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--out", default=os.path.join(HERE, "unet_calls.json"))
    ap.add_argument("--commit", default=None, help="name of the commit whose code is recorded (default: git's HEAD of --root)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from free_hunch_amd import _lib, unet, unet_hip
    commit = a.commit or subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True).strip()
    with patched() as patch:
        queries, traces = record(unet, unet_hip, _lib, patch)
    doc = pack(queries, traces, "every library call of the UNet forward + input-VJP (tests/golden/make_unet_calls.py), written by "
               "unet_hip.py and libfh_hip.so of commit %s" % commit)
    with open(a.out, "w") as f:
        f.write('{"about": %s,\n "configs": %s,\n "queries": [\n' % (json.dumps(doc["about"]), json.dumps(doc["configs"])))
        f.write(",\n".join("  " + json.dumps(q) for q in doc["queries"]))
        f.write('\n ],\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in doc["rows"]))
        f.write('\n ],\n "traces": {\n')
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in doc["traces"].items()))
        f.write("\n }}\n")
    print("%d queries, %d distinct rows, %s calls -> %s" % (len(doc["queries"]), len(doc["rows"]),
                                                             {k: len(v) for k, v in traces.items()}, a.out))


if __name__ == "__main__":
    main()
