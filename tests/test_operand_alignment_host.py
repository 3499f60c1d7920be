"""CPU: the operand-alignment contract of include/diffab_hip.h, as far as it can be held without a device.

  1. `misaligned`, `flat_parameters` and `misalign_parameters` (tests/sampler_support.py) build what they say.
  2. Every (entry, operand) pair of the refusal table (tests/sampler_support.py, mirrored from the header) through the C ABI
     with pointers that are never dereferenced and zero-byte workspaces: a misaligned REFUSED operand gives DIFFAB_ERR_ARG and a message
     naming the entry, the operand and `16-byte`; with every refused operand aligned the call stops at the workspace-size check
     (DIFFAB_ERR_WORKSPACE) instead - whatever the alignment of the ACCEPTED operands.  The alignment check therefore sits among the
     host-side argument checks, in front of the first launch, for every entry of the table.
  3. The Python front end never refuses: _hip.dev_f32 and the weight tables hand the library 16-byte aligned pointers exactly where the
     table says "refused" (a recording stand-in for the library collects the pointers of a whole Denoiser.forward), and dev_i64 /
     dev_mask keep a misaligned view where the table says "accepted".
"""
import ctypes as C
import re

import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from sampler_support import (DEBUG_REFUSES, HOST_NL, LAYER_FIELDS, MESSAGE_NAME, MLP3_FIELDS, SIGNATURES, TABLE_FIELDS, flat_parameters,
                             misalign_parameters, misaligned, refused, signature, table_operands)

FAKE = 1 << 20  # an address nothing is mapped at: every call below returns before it enqueues work


# ---------------------------------------------------------------------------------------------------------------- 1. the helpers
@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (4, 8, 12)), (torch.int64, (8,)), (torch.bool, (1, 3, 15)),
                                           (torch.uint8, (1, 3))])
def test_misaligned_views(dtype, offsets):
    t = (torch.arange(2 * 5 * 3) % 2).reshape(2, 5, 3).to(dtype)
    for off in offsets:
        v = misaligned(t, off)
        assert v.data_ptr() % 16 == off and v.is_contiguous()
        assert v.shape == t.shape and v.dtype == t.dtype and v.device == t.device and torch.equal(v, t)
        assert v.untyped_storage().nbytes() > t.numel() * t.element_size()  # a view of a larger buffer
        v.zero_()
        assert t.any()  # ... of its own: the original is not written through it
    with pytest.raises(AssertionError):
        misaligned(torch.zeros(4), 2)  # not a multiple of the element size
    with pytest.raises(AssertionError):
        misaligned(torch.zeros(4), 16)


def test_flat_parameters_are_views_of_one_shifted_vector():
    """Every parameter becomes a view of one flat vector one float behind a 16-byte boundary, packed in named_parameters() order with
    the values kept; at the benchmark denoiser's shapes the views behind the 3-wide coordinate_denoising.4.bias change residue."""
    from diffab_pytorch.diffab_pytorch import Denoiser

    d = dict(syn.BENCH_DIMS, NL=1)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    before = {n: p.detach().clone() for n, p in den.named_parameters()}
    flat, offs = flat_parameters(den, shift_floats=1)
    assert flat.data_ptr() % 16 == 4 and flat.numel() == sum(v.numel() for v in before.values())
    at = 0
    for n, p in den.named_parameters():
        assert torch.equal(p.data, before[n]) and p.is_contiguous()
        assert p.data_ptr() == flat.data_ptr() + 4 * at and p.data_ptr() % 16 == offs[n]
        at += p.numel()
    assert set(offs.values()) >= {4} and len(set(offs.values())) > 1, offs
    flat.zero_()
    assert all(not p.any() for p in den.parameters())  # one storage
    hit = misalign_parameters(den, lambda n: n.endswith("gamma"), 12)
    assert hit and all(dict(den.named_parameters())[n].data_ptr() % 16 == 12 for n in hit)


# ---------------------------------------------------------------------------------------------------------------- 2. the C ABI
class Call:
    """One entry's argument list with never-dereferenced pointers: every pointer 256-byte aligned until `shift` moves one."""

    def __init__(self, entry):
        self.entry, self.keep, self.ptr, self.args = entry, [], {}, []
        nxt = [FAKE]

        def fresh():
            nxt[0] += 4096
            return nxt[0]

        def table(cls, fields, name, kind):
            obj = cls()
            for f in fields:
                self.ptr[f"{name}.{f}" if kind not in ("LW", "LG") else f"{name}.layers[0].{f}"] = (obj, f)
                setattr(obj, f, fresh())
            return obj

        b = syn.BENCH_DIMS
        for name, kind in signature(entry):
            if kind == "dims":
                v = C.byref(self._hold(_hip.Dims(2, 64, b["D"], b["C"], b["H"], b["DS"], b["PQ"], b["PV"], HOST_NL, 21)))
            elif kind == "cdims":
                v = C.byref(self._hold(_hip.CtxDims(1, 128, 15, 128, 64, 32)))
            elif kind in ("W", "G"):
                layers = self._hold((_hip.IpaLayerWeights * HOST_NL)())
                for l in range(HOST_NL):
                    for f in LAYER_FIELDS:
                        setattr(layers[l], f, fresh())
                        self.ptr[f"{name}.layers[{l}].{f}"] = (layers[l], f)
                w = self._hold(_hip.DenoiserWeights())
                w.layers = C.cast(layers, C.POINTER(_hip.IpaLayerWeights))
                for f in ("seq_emb", "res_w0", "res_b0", "res_w2", "res_b2"):
                    setattr(w, f, fresh())
                    self.ptr[f"{name}.{f}"] = (w, f)
                for h in ("coord", "orient", "seq"):
                    for f in MLP3_FIELDS:
                        setattr(getattr(w, h), f, fresh())
                        self.ptr[f"{name}.{h}.{f}"] = (getattr(w, h), f)
                v = C.byref(w)
            elif kind in ("LW", "LG"):
                v = C.byref(self._hold(table(_hip.IpaLayerWeights, LAYER_FIELDS, name, kind)))
            elif kind in ("RW", "RG"):
                v = C.byref(self._hold(table(_hip.ResidueEmbWeights, TABLE_FIELDS[kind], name, kind)))
            elif kind in ("PW", "PG"):
                v = C.byref(self._hold(table(_hip.PairEmbWeights, TABLE_FIELDS[kind], name, kind)))
            elif kind == "S":
                s = self._hold(_hip.Sched(10, *[fresh() for _ in range(5)]))
                for f in ("alpha", "alpha_bar", "alpha_bar_sqrt", "one_minus_alpha_bar_sqrt", "beta"):
                    self.ptr[f"{name}.{f}:fa"] = (s, f)
                v = C.byref(s)
            elif kind == "I":
                t = self._hold(_hip.Igso3(11, 8, fresh(), fresh(), 0.1))
                for f in ("sigmas", "cdf"):
                    self.ptr[f"{name}.{f}:fa"] = (t, f)
                v = C.byref(t)
            elif kind in ("f", "fa", "i64", "m", "ws"):
                v = None
                self.ptr[name if kind == "f" else f"{name}:{kind}"] = (self.args, len(self.args))
                self.args.append(fresh())
                continue
            elif kind == "tlist":
                v = self._hold((C.c_int32 * 1)(1))
            elif kind in ("null", "N"):
                v = None
            else:
                v = int(kind)
            self.args.append(v)

    def _hold(self, obj):
        self.keep.append(obj)
        return obj

    def shift(self, key, nbytes):
        owner, where = self.ptr[key]
        if isinstance(owner, list):
            owner[where] += nbytes
        else:
            setattr(owner, where, getattr(owner, where) + nbytes)

    def __call__(self):
        lib = _hip.load_library()
        rc = getattr(lib, self.entry)(*self.args)
        return rc, lib.diffab_last_error().decode()


ENTRY_IDS = sorted(SIGNATURES)


@pytest.mark.parametrize("entry", ENTRY_IDS)
def test_refused_operands_are_refused_on_the_host_and_nothing_else_is(entry):
    """Needs no GPU: no pointer is dereferenced, the workspaces are zero bytes, and every outcome below is decided before a launch."""
    who = MESSAGE_NAME.get(entry, entry[len("diffab_"):])
    table = refused()[entry]
    rc, msg = Call(entry)()
    assert rc == -4, (entry, "every operand aligned: the workspace-size check is the one that stops the call", rc, msg)
    assert sorted(table) == sorted(k for k in Call(entry).ptr if ":" not in k), "the driver and the table name the same operands"
    for operand in table:
        for off in (4, 8, 12):
            c = Call(entry)
            c.shift(operand, off)
            rc, msg = c()
            assert rc == -1, (entry, operand, off, rc, msg)
            assert msg.startswith(f"{who}: operand {operand} must be 16-byte aligned"), (entry, operand, msg)
    # every accepted pointer at its natural alignment, all at once: not refused
    c = Call(entry)
    accepted = [k for k in c.ptr if ":" in k and not k.endswith(":ws")]
    assert accepted or "ipa_layer" in entry, entry  # (the layer entries take float operands only)
    for k in accepted:
        c.shift(k, {"fa": 4, "i64": 8, "m": 1}[k.rsplit(":", 1)[1]])
    rc, msg = c()
    assert rc == -4, (entry, "accepted operands misaligned", accepted, rc, msg)
    for k in accepted:  # masks at +3, floats at +12 as well
        c.shift(k, {"fa": 8, "i64": 0, "m": 2}[k.rsplit(":", 1)[1]])
    assert c()[0] == -4, entry
    # and every refused operand at once: refused, naming one of them
    c = Call(entry)
    for operand in table:
        c.shift(operand, 4)
    rc, msg = c()
    assert rc == -1 and re.match(rf"{who}: operand \S+ must be 16-byte aligned", msg), (entry, rc, msg)


def test_refusal_table_names_every_buffer_of_every_weight_table():
    r = refused()
    assert len(r["diffab_denoise_step_fwd"]) == 10 + 5 + 18 + 10 * HOST_NL
    assert "grads.layers[1].w_bias" in r["diffab_train_step_bwd"] and "w.coord.b4" in r["diffab_sample_loop_ex"]
    assert set(r["diffab_sample_loop"]) - set(table_operands("w", "W")) == {"x", "O", "res_ctx", "pair_ctx"}
    assert set(r["diffab_score_designs"]) - set(table_operands("w", "W")) == {"res_ctx", "pair_ctx"}
    assert "g.mw0" in r["diffab_pair_embedding_bwd_taped"] and "w.aa_emb" in r["diffab_residue_embedding_fwd"]


# ---------------------------------------------------------------------------------------------------------------- 3. the front end
class RecordingLibrary:
    """Stands in for libdiffab_hip.so: every call is recorded and returns 0 (a *_bytes query: 256)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 256 if name.endswith("_bytes") else 0

        return fn


def host_front_end(monkeypatch):
    lib = RecordingLibrary()
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_hip, "stream_ptr", lambda: C.c_void_p(0))
    return lib


def address(v):
    return (v.value or 0) if isinstance(v, C.c_void_p) else int(v or 0)


def test_dev_helpers_align_what_would_be_refused_and_keep_what_is_accepted(monkeypatch):
    host_front_end(monkeypatch)
    x = torch.arange(24.0).reshape(2, 4, 3)
    for off in (4, 8, 12):
        v = misaligned(x, off)
        a = _hip.dev_f32(v)
        assert a.data_ptr() % 16 == 0 and a.is_contiguous() and torch.equal(a, x) and a.data_ptr() != v.data_ptr()
    same = _hip.dev_f32(x.clone())
    assert same.data_ptr() % 16 == 0
    al = torch.zeros(64)
    assert _hip.dev_f32(al).data_ptr() == al.data_ptr()  # an aligned tensor is passed as it is: no copy
    s = misaligned(torch.arange(6).reshape(2, 3), 8)
    assert _hip.dev_i64(s).data_ptr() == s.data_ptr()  # int64 and masks are accepted at their natural alignment: no copy
    sliced = torch.zeros(4, 173, 3)[1:3]  # the natural case: a batch slice at a ragged patch length
    assert sliced.is_contiguous() and sliced.data_ptr() % 16 == 12 and _hip.dev_f32(sliced).data_ptr() % 16 == 0
    sched = _hip.SchedOnDevice({k: misaligned(torch.rand(11), 4) for k in ("alpha", "alpha_bar", "alpha_bar_sqrt",
                                                                          "one_minus_alpha_bar_sqrt", "beta")})
    assert all(t.data_ptr() % 16 == 0 for t in sched.tensors.values())


def test_denoiser_forward_hands_the_library_aligned_pointers(monkeypatch):
    """Denoiser.forward on flat-vector parameters and misaligned inputs: every pointer of the diffab_denoise_step_fwd call that the
    table lists as refused is 16-byte aligned, the weight table's buffers included; seq_t (accepted) is the caller's misaligned view."""
    from diffab_pytorch.diffab_pytorch import Denoiser

    lib = host_front_end(monkeypatch)
    d = dict(syn.BENCH_DIMS, NL=HOST_NL)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21).requires_grad_(False)
    _, offs = flat_parameters(den)
    assert any(offs.values())
    B, K = 2, 16
    seq = misaligned(torch.zeros(B, K, dtype=torch.long), 8)
    x, O = misaligned(torch.zeros(B, K, 3), 4), misaligned(torch.eye(3).expand(B, K, 3, 3).contiguous(), 8)
    rc, pc, beta = misaligned(torch.zeros(B, K, d["D"]), 12), misaligned(torch.zeros(B, K, K, d["C"]), 4), misaligned(torch.rand(B), 4)
    den(seq, x, O, rc, pc, beta, return_logits=True)
    name, args = [c for c in lib.calls if c[0] == "diffab_denoise_step_fwd"][0]
    sig = signature(name)
    assert len(sig) == len(args)
    checked = 0
    for (arg, kind), v in zip(sig, args):
        if kind == "f":
            assert address(v) % 16 == 0 and address(v) != 0, arg
            checked += 1
        elif kind == "i64":
            assert address(v) == seq.data_ptr()
        elif kind == "W":
            w = v._obj
            ptrs = [getattr(w, f) for f in ("seq_emb", "res_w0", "res_b0", "res_w2", "res_b2")]
            ptrs += [getattr(getattr(w, h), f) for h in ("coord", "orient", "seq") for f in MLP3_FIELDS]
            ptrs += [getattr(w.layers[l], f) for l in range(HOST_NL) for f in LAYER_FIELDS]
            assert len(ptrs) == len(table_operands("w", "W")) and all(p and p % 16 == 0 for p in ptrs)
            checked += len(ptrs)
    assert checked == len(refused()[name])


def test_debug_gemm_entries_refuse_by_name_before_their_scratch_checks():
    """diffab_debug_linear128 (modes 1 and 2) and diffab_debug_xstat128: every operand of DEBUG_REFUSES at +4 / +8 / +12 is refused by
    name; aligned, the call stops at its scratch check instead (no scratch is given), and mode 0 of linear128 is not on the list."""
    lib = _hip.load_library()
    base = {"X": FAKE, "W": FAKE + 4096, "bias": FAKE + 8192, "Y": FAKE + 12288}
    calls = {"diffab_debug_linear128": lambda p, mode: lib.diffab_debug_linear128(p["X"], p["W"], p["bias"], p["Y"], 64, 128, mode, None, 0, None),
             "diffab_debug_xstat128": lambda p, mode: lib.diffab_debug_xstat128(p["X"], p["W"], p["Y"], 64, 96, mode, FAKE + 16384, 0, None)}
    for entry, operands in DEBUG_REFUSES.items():
        who = entry[len("diffab_"):]
        for mode in (1, 2):
            assert calls[entry](base, mode) == -1 and b": operand " not in lib.diffab_last_error(), (entry, mode, lib.diffab_last_error())
            for operand in operands:
                for off in (4, 8, 12):
                    assert calls[entry](dict(base, **{operand: base[operand] + off}), mode) == -1, (entry, operand, off)
                    assert lib.diffab_last_error().decode().startswith(f"{who}: operand {operand} must be 16-byte aligned"), (entry, operand)
