"""The operand-extent harness and its table on CPU tensors, without a device (include/diffab_hip.h, "Operand extents").

1. The table: WRITES (tests/sampler_support.py) is what the two headers' prototypes and structs leave writable - the non-const pointer
   parameters and struct fields a small parser finds - plus the gradient tables, which the C types cannot mark; both ways, so a new
   export, a new output or a name the headers dropped fails here.  Every entry with a data operand has a case in
   tests/test_gpu_operand_extents.py.
2. GuardedABI: stand-in entries written in Python, under the names and ctypes signatures of real exports, work on the shadows they are
   handed through raw_bytes of the shadow's buffer (as tests/test_scratch_poison_host.py drives `poisoned`).  A well-behaved one
   passes; each kind of violation is reported with the operand, the side and the element offset.
3. Why two fills: a stray store of the value a guard already holds is invisible under that fill, and caught under the other.
"""
import ctypes as C

import pytest
import torch

from diffab_pytorch import _hip
from sampler_support import (ENTRIES, GRADIENT_TABLES, GUARD_BYTES, GUARD_FILLS, HEADERS, NO_DATA, UNGUARDED, WRITES, ConstOperandChanged,
                             GuardDamaged, GuardedABI, UnresolvedPointer, flat_parameters, header_exports, header_prototypes, typed_writes, writable)
from scratch_poison import raw_bytes


# ---------------------------------------------------------------------------------------------------------------- 1. the table
def test_the_parser_reads_both_headers():
    structs, protos = header_prototypes()
    assert sorted(protos) == header_exports() == sorted(set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS))
    assert header_exports(HEADERS[1:]) == ["diffab_metrics_surface"]
    for name, params in protos.items():  # one parameter per ctypes argument, pointers where ctypes has pointers
        args = dict(_hip.SYMBOLS, **_hip.ANALYSIS_SYMBOLS)[name][1]
        assert len(params) == len(args), name
        for (p, base, pointer, const), a in zip(params, args):
            assert pointer == (a is C.c_void_p or hasattr(a, "contents")), (name, p)
    # struct fields by name, in order, as _hip declares them
    for cname, cls in (("diffab_ipa_layer_weights", _hip.IpaLayerWeights), ("diffab_mlp3_weights", _hip.Mlp3Weights),
                       ("diffab_denoiser_weights", _hip.DenoiserWeights), ("diffab_sched", _hip.Sched), ("diffab_igso3", _hip.Igso3),
                       ("diffab_residue_emb_weights", _hip.ResidueEmbWeights), ("diffab_pair_emb_weights", _hip.PairEmbWeights),
                       ("diffab_score_noised", _hip.ScoreNoised), ("diffab_sample_record", _hip.SampleRecord),
                       ("diffab_sample_steps", _hip.SampleSteps), ("diffab_sample_guidance", _hip.SampleGuidance),
                       ("diffab_sample_temperature", _hip.SampleTemperature), ("diffab_sample_steering", _hip.SampleSteering),
                       ("diffab_sample_options", _hip.SampleOptions)):
        assert [f[0] for f in structs[cname]] == [f for f, _ in cls._fields_], cname
    const = {f: c for f, _, _, c in structs["diffab_sample_record"]}
    assert const["slot_of_step"] and not const["slot_dev"] and not const["seq_probs"]
    assert ("coord", "diffab_mlp3_weights", False, False) in structs["diffab_denoiser_weights"]


def test_writes_is_what_the_headers_leave_writable():
    typed = typed_writes()
    assert sorted(WRITES) == sorted(typed), (sorted(set(typed) - set(WRITES)), sorted(set(WRITES) - set(typed)))  # exports, both ways
    assert set(GRADIENT_TABLES) <= set(typed)
    for entry, ops in typed.items():
        listed = WRITES[entry].split()
        assert len(listed) == len(set(listed)), entry
        want = set(ops) | ({GRADIENT_TABLES[entry] + ".*"} if entry in GRADIENT_TABLES else set())
        assert set(listed) == want, (entry, sorted(want - set(listed)), sorted(set(listed) - want))
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes()[1].items()}
    for entry, table in GRADIENT_TABLES.items():  # the exceptions name a parameter that is a weights struct passed as const
        assert table in params[entry] and not any(o.startswith(table + ".") for o in typed[entry]), entry
    assert writable("diffab_train_step_bwd", "grads.layers[1].w_out") and writable("diffab_train_step_bwd", "grads.coord.b4")
    assert not writable("diffab_train_step_bwd", "w.layers[1].w_out") and not writable("diffab_train_step_bwd", "x_t")
    assert writable("diffab_sample_loop_ex", "opt.record.seq_probs") and not writable("diffab_sample_loop_ex", "opt.allowed")
    assert writable("diffab_score_designs", "noised.eps") and not writable("diffab_metrics_surface", "points")
    assert writable("diffab_metrics_surface", "hotspot_buried_area")
    for entry, operand in UNGUARDED:
        assert operand in params[entry] and not writable(entry, operand), (entry, operand)  # only inputs may go unguarded


def test_every_entry_with_a_data_operand_has_a_gpu_case():
    from test_gpu_operand_extents import CASES, COVERED

    data = {n for n, c in ENTRIES.items() if c != NO_DATA}
    assert sorted(ENTRIES) == header_exports()
    assert COVERED == data, (sorted(data - COVERED), sorted(COVERED - data))
    for case, (entries, module, function, fixtures, args) in CASES.items():
        assert entries and all(e in WRITES for e in entries), case


# ---------------------------------------------------------------------------------------------------------------- 2. the harness
def mem(abi, pointer, nbytes):
    """The `nbytes` at the shadow pointer `pointer` as a uint8 view of the shadow's buffer - its guards are in reach, nothing else is."""
    for s in abi.last.values():
        base = s["buf"].data_ptr()
        if base <= pointer < base + s["buf"].numel():
            return raw_bytes(s["buf"])[pointer - base:pointer - base + nbytes]
    raise KeyError(hex(pointer))


def val(p):
    return int((p.value if isinstance(p, C.c_void_p) else p) or 0)


class StandIn:
    """Python entries under real names.  `stray` = (operand bytes, byte offset from the operand's end or, negative, from its start, value
    bytes): one store outside the written operand.  `seen`: the pointers each call was handed."""

    def __init__(self):
        self.abi, self.stray, self.touch_input, self.seen = None, None, None, {}

    def _f32(self, p, n):
        return mem(self.abi, val(p), 4 * n).view(torch.float32)

    def _stray(self, p, nbytes):
        if self.stray is not None:
            off, value = self.stray
            at = val(p) + (nbytes + off if off >= 0 else off)
            mem(self.abi, at, len(value)).copy_(torch.tensor(list(value), dtype=torch.uint8))

    def diffab_so3_log(self, R, S, n, stream):  # S = R + 1
        self.seen["so3_log"] = (val(R), val(S), stream)
        self._f32(S, 9 * n).copy_(self._f32(R, 9 * n) + 1)
        if self.touch_input is not None:
            self._f32(R, 9 * n)[self.touch_input] = -5.0
        self._stray(S, 36 * n)
        return 0

    def diffab_categorical_sample(self, prob, u, n_rows, V, out, stream):  # out = row index
        mem(self.abi, val(out), 8 * n_rows).view(torch.int64).copy_(torch.arange(n_rows))
        self._stray(out, 8 * n_rows)
        return 0

    def diffab_reverse_update_jump(self, s, t, s_next, bj, aj, seq, x, O, eps_hat, O0_hat, posterior, gen_mask, z, rotvec, u_seq, r_out, B, K,
                                   V, stream):  # x += alpha[0]; r_out = 2 * posterior (in place where they alias)
        sched = s._obj
        self.seen["jump"] = dict(posterior=val(posterior), r_out=val(r_out), alpha=sched.alpha, beta=sched.beta)
        self._f32(x, 3 * B * K).add_(self._f32(sched.alpha, 1)[0])
        self._f32(r_out, B * K * V).copy_(2 * self._f32(posterior, B * K * V))
        return 0

    def diffab_denoise_step_fwd(self, d, w, seq_t, x_t, O_t, res_ctx, pair_ctx, beta, out_eps, out_O0, out_posterior, out_logits, out_res_emb,
                                workspace, workspace_bytes, flags, stream):  # out_eps = coord.b4 + layers[1].w_out[0]
        tab, dims = (getattr(v, "_obj", None) or v.contents for v in (w, d))  # (byref or pointer)
        layers = [tab.layers[l] for l in range(dims.NL)]
        self.seen["fwd"] = dict(b4=tab.coord.b4, w_out=layers[1].w_out, workspace=val(workspace))
        self._f32(out_eps, 3).copy_(self._f32(tab.coord.b4, 3) + self._f32(layers[1].w_out, 1)[0])
        if self.stray is not None:
            which, nbytes = self.stray_in
            self._stray(tab.coord.b4 if which == "w.coord.b4" else layers[1].w_out, nbytes)
        return 0

    def diffab_sample_loop_ex(self, d, w, s, rev_tab, seq, x, O, res_ctx, pair_ctx, gen_mask, seed, first_patch, t_start, t_stop, workspace,
                              workspace_bytes, flags, opt, stream):  # record.seq = seq + 1, guidance.shift_dev = allowed[0]
        o = opt._obj
        rec, gd = o.record.contents, o.guidance.contents
        n = d._obj.B * d._obj.K
        self.seen["loop"] = dict(rec_seq=rec.seq, slot_of_step=C.addressof(rec.slot_of_step.contents), allowed=o.allowed, chain=gd.chain)
        mem(self.abi, rec.seq, 8 * n).view(torch.int64).copy_(mem(self.abi, val(seq), 8 * n).view(torch.int64) + 1)
        self._f32(gd.shift_dev, 3 * n).fill_(float(mem(self.abi, o.allowed, 4).view(torch.int32)[0]))
        self._stray(rec.seq, 8 * n)
        return 0

    def diffab_patch_select(self, ca, *rest):
        self.seen["ca"] = val(ca)
        return 0


def guarded(stand, entries, fill, **kw):
    abi = GuardedABI(entries, fill, lib=stand, **kw)
    stand.abi = abi
    return abi


def so3_call(stand, fill, n=5):
    R, S = torch.randn(n, 3, 3), torch.full((n, 3, 3), 9.0)
    R0 = R.clone()
    with guarded(stand, ("diffab_so3_log",), fill) as abi:
        rc = _hip.lib().diffab_so3_log(_hip.ptr(R), _hip.ptr(S), n, None)
    return abi, rc, R, S, R0


@pytest.mark.parametrize("fill", GUARD_FILLS)
def test_a_well_behaved_entry_passes_and_its_output_is_copied_back(fill):
    names = (_hip.lib, _hip.ptr, _hip.workspace)
    stand = StandIn()
    abi, rc, R, S, R0 = so3_call(stand, fill)
    assert rc == 0 and torch.equal(S, R + 1) and torch.equal(R, R0)
    assert abi.counts == {"diffab_so3_log": 2}
    pR, pS, stream = stand.seen["so3_log"]
    assert stream is None and pR != R.data_ptr() and pS != S.data_ptr()
    assert pR % 256 == R.data_ptr() % 256 and pS % 256 == S.data_ptr() % 256  # the entry picks the kernel it would have picked
    assert (_hip.lib, _hip.ptr, _hip.workspace) == names
    assert GUARD_BYTES == 128 * 128 * 4


@pytest.mark.parametrize("fill", GUARD_FILLS)
def test_guard_fills_are_values_of_the_operands_type(fill):
    abi = GuardedABI((), fill, lib=StandIn())
    for dtype, nan0, ones in ((torch.float32, None, 1.0), (torch.float64, None, 1.0), (torch.int64, 0, 1), (torch.int32, 0, 1),
                              (torch.bool, False, True), (torch.uint8, 0, 1)):
        g = abi._pattern(dtype, torch.device("cpu"))
        assert g.dtype == torch.uint8 and g.numel() == GUARD_BYTES
        v = g.view(dtype)
        if fill == "nan0" and nan0 is None:
            assert bool(v.isnan().all()) and bool((g == 0xFF).all())
        else:
            assert bool((v == (nan0 if fill == "nan0" else ones)).all()), (dtype, fill)


def test_aliased_operands_share_one_shadow_and_struct_fields_come_back():
    B, K, V = 2, 3, 21
    tabs = [torch.full((11,), 0.5 + i) for i in range(5)]
    sched = _hip.Sched(10, *[_hip.ptr(t) for t in tabs])  # (built before the context: registered with known=)
    before = [getattr(sched, f) for f, _ in _hip.Sched._fields_]
    seq, x, O = torch.zeros(B, K, dtype=torch.int64), torch.ones(B, K, 3), torch.zeros(B, K, 3, 3)
    post = torch.rand(B, K, V)
    post0, other = post.clone(), [torch.zeros(B, K, 3), torch.zeros(B, K, 3, 3), torch.zeros(B, K, 3), torch.zeros(B, K, 3), torch.zeros(B, K)]
    gm = torch.ones(B, K, dtype=torch.bool)
    stand = StandIn()
    with guarded(stand, ("diffab_reverse_update_jump",), "nan0", known=[tabs]) as abi:
        P = _hip.ptr
        rc = abi.diffab_reverse_update_jump(C.byref(sched), 5, 4, 0.1, 0.9, P(seq), P(x), P(O), P(other[0]), P(other[1]), P(post), P(gm),
                                            P(other[2]), P(other[3]), P(other[4]), P(post), B, K, V, None)
    assert rc == 0
    seen = stand.seen["jump"]
    assert seen["posterior"] == seen["r_out"] != post.data_ptr()  # one address, one shadow: the entry's alias rule still holds
    assert torch.equal(post, 2 * post0) and torch.equal(x, torch.full((B, K, 3), 1.5))  # written through the alias, and copied back
    assert [getattr(sched, f) for f, _ in _hip.Sched._fields_] == before  # the caller's struct is as it was
    assert seen["alpha"] != before[1] and seen["alpha"] % 256 == before[1] % 256 and seen["beta"] != before[5]
    assert abi.counts == {"diffab_reverse_update_jump": 5 + 3 + 5 + 1 + 1}  # the tables, the state, the inputs, the mask, posterior = r_out


@pytest.mark.parametrize("fill", GUARD_FILLS)
@pytest.mark.parametrize("offset, side, where", [(0, "behind", "element 0 behind its end"), (4 * 7, "behind", "element 7 behind its end"),
                                                 (GUARD_BYTES - 4, "behind", f"element {GUARD_BYTES // 4 - 1} behind its end"),
                                                 (-4, "in front of", "element -1 from its start"),
                                                 (-GUARD_BYTES, "in front of", f"element {-GUARD_BYTES // 4} from its start")])
def test_one_element_outside_an_output_is_reported_with_side_and_offset(fill, offset, side, where):
    stand = StandIn()
    stand.stray = (offset, torch.tensor([3.5]).view(torch.uint8).tolist())
    with pytest.raises(GuardDamaged) as err:
        so3_call(stand, fill)
    msg = str(err.value)
    assert "diffab_so3_log: operand S " in msg and f"out of bounds {side} it" in msg and where in msg and f'"{fill}"' in msg, msg


@pytest.mark.parametrize("fill", GUARD_FILLS)
def test_a_changed_const_operand_is_reported_with_its_element(fill):
    stand = StandIn()
    stand.touch_input = 13
    with pytest.raises(ConstOperandChanged) as err:
        so3_call(stand, fill)
    assert "diffab_so3_log: operand R " in str(err.value) and "first changed element 13 of 45" in str(err.value), str(err.value)


def denoiser_tables(NL=2):
    """Dims and a denoiser weights struct over small CPU tensors of their own: (dims, struct, {operand: tensor}, what must stay alive)."""
    t, keep = {}, []

    def table(cls, path):
        s = cls()
        for f, ftype in cls._fields_:
            if ftype is C.c_void_p:
                t[f"{path}.{f}"] = torch.randn(3 + len(t))
                setattr(s, f, t[f"{path}.{f}"].data_ptr())
        return s

    layers = (_hip.IpaLayerWeights * NL)(*[table(_hip.IpaLayerWeights, f"w.layers[{l}]") for l in range(NL)])
    w = table(_hip.DenoiserWeights, "w")
    w.layers = C.cast(layers, C.POINTER(_hip.IpaLayerWeights))
    for head in ("coord", "orient", "seq"):
        setattr(w, head, table(_hip.Mlp3Weights, f"w.{head}"))
    keep.append(layers)
    return _hip.make_dims(2, 4, 8, 4, 2, 4, 2, 2, NL), w, t, keep


def forward_call(stand, fill, known=None, workspace=False):
    d, w, t, keep = denoiser_tables()
    ins = [torch.zeros(2, 4, dtype=torch.int64)] + [torch.zeros(3) for _ in range(5)]
    outs = [torch.zeros(3) for _ in range(5)]
    with guarded(stand, ("diffab_denoise_step_fwd",), fill, known=[t] if known is None else known) as abi:
        ws = _hip.workspace(512) if workspace else None
        rc = abi.diffab_denoise_step_fwd(C.byref(d), C.byref(w), *[_hip.ptr(v) for v in ins + outs], _hip.ptr(ws), 512, 0, None)
    return abi, rc, w, t, outs, ws


@pytest.mark.parametrize("fill", GUARD_FILLS)
def test_nested_structs_and_the_layer_array_are_shadowed(monkeypatch, fill):
    stand = StandIn()
    monkeypatch.setattr(_hip, "device", lambda: torch.device("cpu"))  # (_hip.workspace allocates on the current GPU)
    abi, rc, w, t, outs, ws = forward_call(stand, fill, workspace=True)
    seen = stand.seen["fwd"]
    assert rc == 0 and torch.equal(outs[0], t["w.coord.b4"][:3] + t["w.layers[1].w_out"][0])
    assert seen["b4"] != t["w.coord.b4"].data_ptr() and seen["w_out"] != t["w.layers[1].w_out"].data_ptr()
    assert w.coord.b4 == t["w.coord.b4"].data_ptr() and w.layers[1].w_out == t["w.layers[1].w_out"].data_ptr()  # put back
    assert seen["workspace"] == ws.data_ptr()  # _hip.workspace buffers pass as they are: scratch_poison owns them
    assert abi.counts == {"diffab_denoise_step_fwd": len(t) + 6 + 5}


@pytest.mark.parametrize("fill", GUARD_FILLS)
@pytest.mark.parametrize("operand", ["w.coord.b4", "w.layers[1].w_out"])
def test_a_store_behind_a_table_buffer_is_reported_by_its_path(fill, operand):
    stand = StandIn()
    d, w, t, keep = denoiser_tables()
    stand.stray, stand.stray_in = (8, [1, 2, 3, 4]), (operand, 4 * t[operand].numel())
    with pytest.raises(GuardDamaged) as err:
        forward_call(stand, fill)
    msg = str(err.value)
    assert f"diffab_denoise_step_fwd: operand {operand} " in msg and "behind it" in msg and "element 2 behind its end" in msg, msg


@pytest.mark.parametrize("stray", [None, (16, [7] * 8)])
def test_structs_behind_pointer_fields_are_shadowed(stray):
    """SampleOptions.record / .guidance: device pointers two structs away from the argument; host arrays (slot_of_step) pass."""
    B, K = 2, 4
    d, w, t, keep = denoiser_tables()
    d.B, d.K = B, K
    tabs = [torch.zeros(11) for _ in range(7)]
    sched, rev = _hip.Sched(10, *[_hip.ptr(v) for v in tabs[:5]]), _hip.Igso3(11, 1, _hip.ptr(tabs[5]), _hip.ptr(tabs[6]), 0.1)
    seq, x, O = torch.arange(B * K).view(B, K), torch.zeros(B, K, 3), torch.zeros(B, K, 3, 3)
    ctx, gm = [torch.zeros(B, K, 8), torch.zeros(B, K, K, 4)], torch.ones(B, K, dtype=torch.bool)
    rec_seq, slot_dev, shift = torch.zeros(B, 1, K, dtype=torch.int64), torch.zeros(11, dtype=torch.int32), torch.zeros(B, K, 3)
    rec_x, rec_O = torch.zeros(B, 1, K, 3), torch.zeros(B, 1, K, 3, 3)
    allowed, chain = torch.full((B, K), 5, dtype=torch.int32), torch.zeros(B, K, dtype=torch.int32)
    slots = (C.c_int32 * 11)(*range(11))
    stand = StandIn()
    stand.stray = stray
    with guarded(stand, ("diffab_sample_loop_ex",), "ones", known=[t, tabs]) as abi:
        P = _hip.ptr
        rec = _hip.SampleRecord(1, slots, P(slot_dev), P(rec_seq), P(rec_x), P(rec_O), None, None, None)
        gd = _hip.SampleGuidance(1.0, 3.0, 1.0, 3.8, 0.5, 100, P(chain), P(chain), None, P(shift))
        opt = _hip.SampleOptions(allowed=P(allowed), record=rec, guidance=gd)
        call = lambda: abi.diffab_sample_loop_ex(C.byref(d), C.byref(w), C.byref(sched), C.byref(rev), P(seq), P(x), P(O), P(ctx[0]), P(ctx[1]),  # noqa: E731
                                                 P(gm), 1, 0, 5, 4, None, 0, 0, C.byref(opt), None)
        if stray is None:
            assert call() == 0
        else:
            with pytest.raises(GuardDamaged) as err:
                call()
            assert "diffab_sample_loop_ex: operand opt.record.seq " in str(err.value) and "element 2 behind its end" in str(err.value)
            return
    seen = stand.seen["loop"]
    assert torch.equal(rec_seq.view(B, K), seq + 1) and bool((shift == 5.0).all())  # written through two structs, copied back
    assert seen["rec_seq"] != rec_seq.data_ptr() and seen["allowed"] != allowed.data_ptr() and seen["chain"] != chain.data_ptr()
    assert seen["slot_of_step"] == C.addressof(slots)  # a host array is not a device pointer
    assert opt.record.contents.seq == rec_seq.data_ptr() and opt.allowed == allowed.data_ptr() and opt.guidance.contents.chain == chain.data_ptr()
    # weights 43, schedule 5, table 2, state 3, contexts 2, mask 1, allowed 1, record 4, guidance chain = residue_idx 1 and shift 1
    assert abi.counts == {"diffab_sample_loop_ex": len(t) + 5 + 2 + 3 + 2 + 1 + 1 + 4 + 2}


def test_an_unresolved_device_pointer_fails_unless_it_is_listed():
    stand = StandIn()
    stranger = torch.zeros(5, 3, 3)  # never seen by _hip.ptr, not in known=
    S = torch.zeros(5, 3, 3)
    with pytest.raises(UnresolvedPointer) as err:
        with guarded(stand, ("diffab_so3_log",), "nan0") as abi:
            abi.diffab_so3_log(C.c_void_p(stranger.data_ptr()), _hip.ptr(S), 5, None)
    assert "diffab_so3_log: operand R " in str(err.value) and "UNGUARDED" in str(err.value)
    inner = torch.zeros(5, 4, 3)[:, 1]  # a strided view: seen, but no contiguous extent to copy
    with pytest.raises(UnresolvedPointer):
        with guarded(stand, ("diffab_so3_log",), "nan0") as abi:
            abi.diffab_so3_log(_hip.ptr(inner), _hip.ptr(S), 5, None)
    # the one listed pointer passes as it is
    assert list(UNGUARDED) == [("diffab_patch_select", "ca")]
    with guarded(stand, ("diffab_patch_select",), "nan0") as abi:
        rc = abi.diffab_patch_select(C.c_void_p(stranger.data_ptr() + 12), 12, *[None] * 5, 1, 5, 2, 0, 2, None, None, None, None)
    assert rc == 0 and stand.seen["ca"] == stranger.data_ptr() + 12 and abi.counts == {"diffab_patch_select": 0}
    # an entry that is not listed in `entries` is the library's own
    with guarded(stand, (), "nan0") as abi:
        assert abi.diffab_so3_log.__self__ is stand


def test_the_operand_itself_goes_before_a_buffer_it_is_cut_from():
    """One address, several tensors: the one _hip.ptr sees inside the context wins over known=, and of two known= tensors the smaller -
    so the guard lies directly behind the operand.  A store one element behind the slice is caught whichever way they were registered."""
    n = 5
    for order in ("whole first", "slice first", "seen"):
        whole = torch.zeros(4 * n, 3, 3)
        S, R = whole[:n], torch.randn(n, 3, 3)
        known = {"whole first": [whole, S, R], "slice first": [S, whole, R], "seen": [whole]}[order]
        stand = StandIn()
        stand.stray = (0, [1, 2, 3, 4])
        with pytest.raises(GuardDamaged) as err:
            with guarded(stand, ("diffab_so3_log",), "nan0", known=known) as abi:
                if order == "seen":
                    abi.diffab_so3_log(_hip.ptr(R), _hip.ptr(S), n, None)
                else:
                    abi.diffab_so3_log(C.c_void_p(R.data_ptr()), C.c_void_p(S.data_ptr()), n, None)
        assert "operand S " in str(err.value) and "element 0 behind its end (operand of 45 elements" in str(err.value), (order, str(err.value))


def test_a_freed_workspaces_address_is_an_operand_again(monkeypatch):
    monkeypatch.setattr(_hip, "device", lambda: torch.device("cpu"))
    R, S = torch.randn(5, 3, 3), torch.zeros(5, 3, 3)
    stand = StandIn()
    with guarded(stand, ("diffab_so3_log",), "ones") as abi:
        ws = _hip.workspace(300)
        assert abi.scratch == {ws.data_ptr(): 300}
        _hip.ptr(ws)
        assert ws.data_ptr() in abi.scratch  # the workspace itself stays one
        abi.scratch[S.data_ptr()] = 300  # as if a workspace that is gone had lived where S lives now
        abi.diffab_so3_log(_hip.ptr(R), _hip.ptr(S), 5, None)
        assert S.data_ptr() not in abi.scratch
    assert stand.seen["so3_log"][1] != S.data_ptr() and abi.counts == {"diffab_so3_log": 2} and torch.equal(S, R + 1)


def test_the_layer_count_is_read_from_a_dims_pointer_too():
    stand = StandIn()
    d, w, t, keep = denoiser_tables()
    ins = [torch.zeros(2, 4, dtype=torch.int64)] + [torch.zeros(3) for _ in range(5)]
    outs = [torch.zeros(3) for _ in range(5)]
    with guarded(stand, ("diffab_denoise_step_fwd",), "nan0", known=[t]) as abi:
        abi.diffab_denoise_step_fwd(C.pointer(d), C.pointer(w), *[_hip.ptr(v) for v in ins + outs], None, 0, 0, None)
    assert stand.seen["fwd"]["w_out"] != t["w.layers[1].w_out"].data_ptr() and abi.counts == {"diffab_denoise_step_fwd": len(t) + 11}


# ---------------------------------------------------------------------------------------------------------------- 3. why two fills
def test_a_stray_zero_behind_an_int64_output_needs_the_other_fill():
    def run(fill):
        stand = StandIn()
        stand.stray = (0, [0] * 8)  # the int64 0 one element behind `out`: exactly what the "nan0" guard holds there
        prob, u, out = torch.rand(6, 21), torch.rand(6), torch.zeros(6, dtype=torch.int64)
        with guarded(stand, ("diffab_categorical_sample",), fill) as abi:
            abi.diffab_categorical_sample(_hip.ptr(prob), _hip.ptr(u), 6, 21, _hip.ptr(out), None)
        assert torch.equal(out, torch.arange(6))

    run("nan0")
    with pytest.raises(GuardDamaged) as err:
        run("ones")
    assert "operand out " in str(err.value) and "element 0 behind its end" in str(err.value) and "value 0x00" in str(err.value)


def test_unknown_fill_is_refused():
    with pytest.raises(ValueError):
        GuardedABI((), "a5")


# ---------------------------------------------------------------------------------------------------------------- 4. flat vectors
@pytest.mark.parametrize("shift, align", [(0, 4), (1, 1), (3, 4)])
def test_flat_parameters_with_gradients_lays_out_views_and_fill(shift, align):
    """The layout the flat-vector GPU case relies on: values kept, zero gradients in views of one vector, every view at a multiple of
    `align` floats from a start `shift` floats behind a 16-byte boundary, and outside() exactly the bytes no view covers, all at the fill."""
    torch.manual_seed(3)
    m = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.randn(*shape)) for k, shape in
                                (("a", (3,)), ("b", (4, 2)), ("c", (21,)), ("d", (2, 3, 2)), ("e", (5,)))})
    values = {n: p.detach().clone() for n, p in m.named_parameters()}
    flat, offs, gflat, outside = flat_parameters(m, shift_floats=shift, grads=7.25, align_floats=align)
    sizes = [p.numel() for _, p in m.named_parameters()]
    at, starts = 0, []
    for n_ in sizes:
        at = (at + align - 1) // align * align
        starts.append(at)
        at += n_
    assert flat.numel() == gflat.numel() == at and flat.data_ptr() % 16 == gflat.data_ptr() % 16 == 4 * shift
    for (n, p), lo in zip(m.named_parameters(), starts):
        assert torch.equal(p.data, values[n]) and p.grad.shape == p.shape and not p.grad.any()
        assert p.data_ptr() == flat.data_ptr() + 4 * lo and p.grad.data_ptr() == gflat.data_ptr() + 4 * lo
        assert offs[n] == p.data_ptr() % 16 and (align != 4 or offs[n] == 4 * shift)
    for vec in (flat, gflat):
        out = outside(vec)
        assert out.numel() == raw_bytes(vec).numel() - 4 * sum(sizes) and out.numel() >= 32 + 4 * (at - sum(sizes))
        assert bool((out.view(torch.float32) == 7.25).all())
    # a store one float behind a view, into padding or in front of the whole vector, shows in outside(); one inside a view does not
    clean = outside(gflat).clone()
    m["c"].grad.add_(1.0)
    assert torch.equal(outside(gflat), clean)
    raw_bytes(gflat).view(torch.float32)[gflat.storage_offset() - 1] = 0.0
    assert not torch.equal(outside(gflat), clean)
    if align == 4:
        flat2, _, gflat2, outside2 = flat_parameters(m, shift_floats=shift, grads=7.25, align_floats=align)
        clean2 = outside2(gflat2).clone()
        gflat2[3] = 0.0  # the float of padding behind the 3-wide "a"
        assert not torch.equal(outside2(gflat2), clean2)
    # the old form is unchanged: two values, parameters back to back
    flat3, offs3 = flat_parameters(m)
    assert flat3.numel() == sum(sizes) and flat3.data_ptr() % 16 == 4 and all(torch.equal(p.data, values[n]) for n, p in m.named_parameters())
