"""What an entry may do to its caller's streams (include/diffab_hip.h, "Streams"): every launch and copy goes on `stream`, or on an
internal stream ordered after and before `stream` by events; no entry waits on the host; a HOST array is dead to the library on return.

Every other test hands the library the legacy default stream with nothing in front of it: a kernel launched on 0 instead of `stream`, a
memset on the wrong stream, a side stream forked from the wrong event and a helper that drains the device all give the right numbers
there.  Here every entry runs on a side stream that is busy (GatedStreamABI, tests/sampler_support.py): operands are shadows that hold
decoys until the gate has ended, so work that does not wait for the gate computes on decoys or is overwritten, and a call that waits on
the host returns after the gate instead of during it.

No new numerical reference.  ROWS are the rows of tests/test_gpu_operand_extents.py (every entry with a data operand, one row per
kernel path at the smallest shape) and one row per export of the seven later headers: an existing test function - its float64 oracle
or restatement, its bounds - rerun on top of the harness.  The HOST-array cases call through the front end and overwrite the array the
moment the entry returns.  Three stand-in entries written in Python prove that the harness can fail.
"""
import ctypes as C
import importlib
import time

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, metrics
from sampler_support import (CTX, HOST_ARRAYS, MAY_WAIT, STATE, EntryWaited, GatedStreamABI, assert_bitwise, gated_stream, hip,  # noqa: F401
                             patches, rows, sample, tensors_of, unit_model)
from test_gpu_aa_constraints import unit as aa_unit  # noqa: F401  (fixtures of the rerun tests, under names of their own)
from test_gpu_operand_extents import CASES as EXTENT_CASES, TRAIN
from test_gpu_respaced import bench as respaced_bench  # noqa: F401
from test_gpu_reverse_step_composed import empty_set_reaches_the_kernel, models as composed_models  # noqa: F401
from test_gpu_reverse_step_composed import steered_models  # noqa: F401
from test_gpu_score import unit as score_unit  # noqa: F401
from test_gpu_steering import unit as steering_unit  # noqa: F401

pytestmark = pytest.mark.gpu
GATE = True  # (False: everything but the gate - how the ungated host times of profiles/stream_contract.md were taken)

# Rows of the extent test that repeat a kernel path of a smaller row of the same entry: row -> the row that stays
DROPPED = {"forward_k173_dispatch": "forward_k37_dispatch", "forward_k173_pairplanes": "forward_k37_pairplanes",  # the generic forward
           "forward_k256_dispatch": "forward_k192_dispatch", "forward_k256_pairplanes": "forward_k192_pairplanes",  # MFMA, key chunks
           "forward_groups_k64_pairplanes": "forward_groups_k64", "train_k64_b3": "train_k64_nl7", "cotangents_k196": "cotangents_k173",
           "sample_loop_plain_k173": "sample_loop_plain_k128", "layer_forward_k192": "layer_forward_k173",
           "xstat128_129x1344": "xstat128_300x100"}
ROWS = {k: v for k, v in EXTENT_CASES.items() if k not in DROPPED}
# The twelve exports of the seven later headers: the smallest case of each one's own test that is more than one work item
ROWS.update({
    # (hbonds, cluster, pareto: the oracle cases of these three files carve their operands out of one arena; their front-end tests hold
    # the same oracle and hand the library tensors of their own)
    "hbonds": (("diffab_metrics_hbonds",), "test_gpu_hbonds", "test_the_python_entry", (), (True, True, True)),
    "cluster": (("diffab_metrics_cluster",), "test_gpu_cluster", "test_the_python_entry", (), ("G3 N129",)),
    "pareto": (("diffab_metrics_pareto",), "test_gpu_pareto", "test_the_python_entry", (), ("N129 M3",)),
    "contact_bits": (("diffab_metrics_contact_bits",), "test_gpu_interface", "test_contact_map_equals_the_restatement", (), (33, 1, True)),
    "pairwise_bits": (("diffab_metrics_pairwise_bits",), "test_gpu_interface", "test_pairwise_bits_equals_the_restatement", (), (2, 3, 5)),
    "patches": (("diffab_metrics_patches",), "test_gpu_developability", "test_patches_equal_the_restatement", (), (33, 1, True, True)),
    "motifs": (("diffab_metrics_motifs",), "test_gpu_developability", "test_liabilities_equal_the_restatement", (), (33, 1)),
    "pair_energy": (("diffab_metrics_pair_energy",), "test_gpu_pair_energy", "test_a_dyadic_table_equals_the_restatement_bit_for_bit", (),
                    (33, 1, True)),
    "edit_nearest": (("diffab_metrics_edit_nearest",), "test_gpu_novelty", "test_extents_and_row_strides_that_are_no_multiple_of_four", (),
                     (65, 63)),
    "pack_sequences": (("diffab_metrics_pack_sequences",), "test_gpu_novelty", "test_pack_sequences_equals_a_gather", (), (65,)),
    "dihedral_nearest": (("diffab_metrics_dihedral_nearest",), "test_gpu_conformation", "test_grid_features_equal_the_restatement_bit_for_bit",
                         (), (2, 15, 63, 64, 64)),
    "pack_dihedrals": (("diffab_metrics_pack_dihedrals",), "test_gpu_conformation", "test_pack_dihedrals_equals_a_gather", (), (65,)),
})
# The known-answer test of the jump update calls its entry for every pair s < t - 1 of a hundred steps, 4 950 times: every call is held to
# its answers, 26 of them run behind the gate (the arguments t, s of the entry: t a multiple of 25, s a multiple of 10).
WHEN = {"diffab_reverse_update_jump": lambda args: int(args[1]) % 25 == 0 and int(args[2]) % 10 == 0}
DRIVEN = {e: row for row in sorted(ROWS, reverse=True) for e in ROWS[row][0]}  # entry -> a row that drives it


def forget_cached_device_results(mod):
    """The analysis test files keep device results of a case in lru_caches (device_energy, device_motifs, ...): a rerun must call the
    entry again.  Inputs and references stay cached."""
    for name, v in vars(mod).items():
        if name.startswith("device") and hasattr(v, "cache_clear"):
            v.cache_clear()


def report(case, abi):
    per = {}
    for entry, early, gate_ms, host_ms, attempts, may_wait in abi.calls:
        p = per.setdefault(entry, dict(calls=0, host_ms=0.0, gate_ms=0.0, late=0, repeated=0, may_wait=0))
        p["calls"] += 1
        p["host_ms"], p["gate_ms"] = max(p["host_ms"], host_ms), max(p["gate_ms"], gate_ms)
        p["late"] += not early
        p["repeated"] += attempts > 1
        p["may_wait"] += may_wait
    for entry, p in per.items():
        print(f"STREAM_CONTRACT {case} {entry} calls={p['calls']} max_host_ms={p['host_ms']:.3f} max_gate_ms={p['gate_ms']:.1f} "
              f"returned_late={p['late']} repeated={p['repeated']} may_wait={p['may_wait']} gate={'on' if abi.gate else 'off'}")
    return per


def assert_returned_early(case, abi):
    """Every gated call returned while the gate was still running - but for the calls MAY_WAIT lists, with its reason."""
    for entry, early, gate_ms, host_ms, attempts, may_wait in abi.calls:
        assert early or may_wait or not abi.gate, (case, entry, "waited on the host", gate_ms, host_ms)
        assert not may_wait or entry in MAY_WAIT


# ---------------------------------------------------------------------------------------------------------------- 1. reruns
@pytest.mark.parametrize("case", sorted(ROWS))
def test_entries_rerun_their_own_reference_test_behind_a_busy_stream(request, case):
    """The test an entry's own file holds, rerun with the entry on a side stream behind a gate and every operand a shadow that holds a
    decoy until the gate has ended: the test's own comparison, every listed entry called on shadows, every call back before the gate
    ended."""
    entries, module, function, fixtures, args = ROWS[case]
    mod = importlib.import_module(module)
    args = args(mod) if callable(args) else args
    values = {f: request.getfixturevalue(f) for f in fixtures}  # (models are built on the real library, before the stand-in)
    known = tensors_of([v for f, v in values.items() if f != "hip"], vars(mod), depth=6)  # tables cached before the harness stands in
    forget_cached_device_results(mod)
    t0 = time.perf_counter()
    with GatedStreamABI(entries, known=known, when=WHEN, gate=GATE) as abi:
        if "hip" in values:
            values["hip"] = abi
        getattr(mod, function)(*[values[f] for f in fixtures], *args)
    forget_cached_device_results(mod)
    report(case, abi)
    print(f"{case}: {time.perf_counter() - t0:.1f} s, operands replaced {abi.counts}")
    for e in entries:
        assert abi.counts.get(e, 0) > 0, (case, e, "was not called on shadows", abi.counts)
    assert_returned_early(case, abi)


# ---------------------------------------------------------------------------------------------------------------- 2. HOST arrays
def overwrite(array, values):
    """array: a ctypes array, or a pointer to one; values: as many numbers as the library was told to read."""
    for i, v in enumerate(values):
        array[i] = v


class HostArrayCase:
    """One front-end call under the gate whose HOST array is overwritten the moment the entry returns: `entry`, `find` ({parameter:
    argument} -> the array), `other` (the valid values it is overwritten with)."""

    def __init__(self, entry, find, other, known=()):
        self.entry, self.find, self.other, self.known, self.overwritten = entry, find, other, known, 0

    def hook(self, named):
        array = self.find(named)
        assert array is not None and bool(array), (self.entry, "the call passed no such array")
        before = [array[i] for i in range(len(self.other))]
        assert before != list(self.other), (self.entry, "the overwrite would change nothing", before)
        overwrite(array, self.other)
        self.overwritten += 1

    def run(self, call):
        with GatedStreamABI((self.entry,), known=self.known, on_return={self.entry: self.hook}, gate=GATE) as abi:
            out = call()
        report(f"host array of {self.entry}", abi)
        assert self.overwritten >= 1 and abi.counts.get(self.entry, 0) > 0, (self.entry, self.overwritten, abi.counts)
        assert_returned_early(self.entry, abi)
        return out


def options(named):
    return named["opt"]._obj if hasattr(named["opt"], "_obj") else named["opt"].contents


@pytest.fixture(scope="module")
def loop_case(hip):
    """The unit model (NL = 2), two contexts at K = 16 and eight steps of the reverse loop: the smallest shared-context sampler case."""
    dims, model, _ = unit_model()
    inp = patches(2, 16, dims, seed=44)
    inp["generation_mask"][:, 3:11] = True
    return model, inp, dict(seed=11, t_start=30, t_stop=22)


def test_ctx_of_row_is_dead_on_return(loop_case):
    """sample(num_samples = 3) is bitwise the replicated batch (tests/test_gpu_shared_context.py) although every entry of ctx_of_row
    is 0 from the moment the loop has returned."""
    model, inp, kw = loop_case
    N, B = 3, inp["seq_idx"].shape[0]
    want = sample(model, rows(inp, torch.arange(B, device="cuda").repeat_interleave(N)), **kw)
    case = HostArrayCase("diffab_sample_loop_ex", lambda a: options(a).ctx_of_row, [0] * (B * N), known=tensors_of(model))
    got = case.run(lambda: sample(model, inp, num_samples=N, **kw))
    assert_bitwise(got, want, "ctx_of_row overwritten on return")


def test_slot_of_step_is_dead_on_return(loop_case):
    """The recorded trajectory is bitwise the ungated call's, and the final state the plain run's (tests/test_gpu_trajectory.py),
    although slot_of_step says `not recorded` everywhere from the moment the loop has returned."""
    model, inp, kw = loop_case
    plain = sample(model, inp, **kw)
    want = sample(model, inp, trajectory=[30, 27, 23], trajectory_predictions=True, **kw)
    case = HostArrayCase("diffab_sample_loop_ex", lambda a: options(a).record.contents.slot_of_step, [-1] * 101, known=tensors_of(model))
    got = case.run(lambda: sample(model, inp, trajectory=[30, 27, 23], trajectory_predictions=True, **kw))
    assert_bitwise(got, want, "slot_of_step overwritten on return")
    assert_bitwise({k: v for k, v in got.items() if k != "trajectory"}, plain, "recording is invisible")
    assert got["trajectory"]["t"].tolist() == [30, 27, 23]


def test_graph_sampler_behind_the_gate_is_the_eager_loop(loop_case):
    """DIFFAB_FLAG_GRAPH_SAMPLER replays a captured step on a private stream that is forked from `stream` by an event and drained before
    the call returns: the call may hold the host (MAY_WAIT), and its samples are bitwise the eager loop's (tests/test_gpu_respaced.py,
    tests/test_gpu_shared_context.py) although the caller's stream was busy when the private stream was forked."""
    model, inp, kw = loop_case
    want = sample(model, inp, **kw)
    with GatedStreamABI(("diffab_sample_loop_ex",), known=tensors_of(model), gate=GATE) as abi:
        got = sample(model, inp, graph=True, **kw)
    report("graph sampler", abi)
    assert [c[5] for c in abi.calls] == [True], abi.calls  # the one call carried the flag
    assert_returned_early("graph sampler", abi)
    assert_bitwise(got, want, "graph replay behind the gate")


@pytest.mark.parametrize("field", ["steps", "beta_jump", "alpha_jump"])
def test_the_step_list_and_its_coefficients_are_dead_on_return(loop_case, field):
    """steps = every step of the range is bitwise the ordinary loop (tests/test_gpu_respaced.py) although, from the moment the loop has
    returned, the step list is another valid list (8, 7, ..., 1) or the jump coefficients are 0.5 everywhere."""
    model, inp, kw = loop_case
    plain = sample(model, inp, **kw)
    other = {"steps": list(range(8, 0, -1)), "beta_jump": [0.5] * 101, "alpha_jump": [0.5] * 101}[field]
    case = HostArrayCase("diffab_sample_loop_ex", lambda a: getattr(options(a).steps.contents, field), other, known=tensors_of(model))
    got = case.run(lambda: sample(model, inp, steps=list(range(30, 22, -1)), **kw))
    assert_bitwise(got, plain, f"{field} overwritten on return")


@pytest.mark.parametrize("operand", ["ctx_of_design", "t_list"])
def test_the_scorer_s_host_arrays_are_dead_on_return(score_unit, operand):
    """DiffAb.score of four designs from two shared contexts on the grid (1, 7, 30): every term against the oracle on the device's own
    noised state (check_terms of tests/test_gpu_score.py) although ctx_of_design is all 0, or t_list (99, 98, 97), from the moment
    the entry has returned."""
    import test_gpu_score as sc

    dims, model = score_unit
    n_ctx, R, K, grid = 2, 4, 16, [1, 7, 30]
    ctx = patches(n_ctx, K, dims, seed=31)
    ci = torch.arange(R) % n_ctx
    inp = {k: ctx[k][ci.cuda()].clone() for k in STATE}
    inp["generation_mask"][:, 2:10] = True
    other = {"ctx_of_design": [0] * R, "t_list": [99, 98, 97]}[operand]
    case = HostArrayCase("diffab_score_designs", lambda a: a[operand], other, known=tensors_of(model))
    out = case.run(lambda: model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                                       res_context_emb=ctx["res_context_emb"], pair_context_emb=ctx["pair_context_emb"], context_index=ci,
                                       t=grid, seed=9, per_residue=True, return_noised=True))
    assert out["t"].tolist() == grid
    full = dict(inp, **{k: ctx[k][ci.cuda()] for k in CTX})
    sc.check_terms(model, dims, full, out, torch.arange(R, device="cuda"), range(len(grid)), 1)


def test_bin_edges_are_dead_on_return(hip):
    """metrics.interface_energy at K = 33 equals the restatement bit for bit (tests/test_gpu_pair_energy.py) although the bin edges
    are (0, 1, 2, 3) from the moment the entry has returned."""
    import test_gpu_pair_energy as pe

    c, want = pe.case(33, 1), pe.reference(33, 1, True)
    case = HostArrayCase("diffab_metrics_pair_energy", lambda a: C.cast(a["bin_edges"], C.POINTER(C.c_float)), [0.0, 1.0, 2.0, 3.0])
    out = case.run(lambda: pe.numpy_of(pe.device_call(c, True, pe.table_of("dyadic", 3, 20), 3)))
    pe.check(out, want, "bin_edges overwritten on return", exact=True)


def test_motifs_are_dead_on_return(hip):
    """metrics.liabilities at K = 33 equals the restatement (tests/test_gpu_developability.py) although the motif words are those of
    the motifs in reverse order from the moment the entry has returned."""
    import test_gpu_developability as dv

    m, want = dv.motif_case(33, 1), dv.motif_reference(33, 1)
    other = [int(v) for v in dv.MOTIF_WORDS[::-1].flatten()]
    case = HostArrayCase("diffab_metrics_motifs", lambda a: C.cast(a["motifs"], C.POINTER(C.c_int32)), other)
    out = case.run(lambda: dv.numpy_of(metrics.liabilities(m["designs"], m["gen_d"], chain_idx=m["chain_d"], residue_idx=m["ridx_d"],
                                                           residue_mask=m["rm_d"], group_size=1)))
    dv.check_motifs(out, want, list(metrics.LIABILITY_MOTIFS), "motifs overwritten on return")


def test_point_radius_is_dead_on_return(hip):
    """metrics.surface at K = 24, S = 33 equals the oracle (tests/test_gpu_surface.py) although every atom radius is 1.0 from the
    moment the entry has returned."""
    import test_gpu_surface as sf

    c, ref = sf.case(24, 8, False, 1, True), sf.reference(24, 8, False, 1, True, 33)
    case = HostArrayCase("diffab_metrics_surface", lambda a: a["point_radius"], [1.0] * len(sf.RADII5))
    out = case.run(lambda: sf.run(c, 33))
    sf.check(out, ref, "point_radius overwritten on return")


def test_complex_of_row_is_dead_on_return(hip):
    """diffab_patch_gather through the row map equals torch indexing (exact) although the map is all 0 from the moment the entry has
    returned."""
    from diffab_pytorch import patch as dpatch

    B, N, K, width = 3, 11, 5, 8
    g = torch.Generator().manual_seed(6)
    src = torch.randn(B, N, width, generator=g)
    cor = [2, 0, 1, 2]
    index = torch.stack([torch.randperm(N, generator=g)[:K] for _ in cor])
    index[1, 2] = -1  # (an unused slot: zero-filled)
    want = torch.stack([torch.where((index[r] >= 0)[:, None], src[b, index[r].clamp_min(0)], torch.zeros(())) for r, b in enumerate(cor)])
    src_d, index_d = src.cuda(), index.cuda()
    case = HostArrayCase("diffab_patch_gather", lambda a: a["complex_of_row"], [0] * len(cor))
    got = case.run(lambda: dpatch._gather_rows(_hip.lib(), src_d, index_d, complex_of_row=cor))
    assert torch.equal(got.cpu(), want)


def test_every_host_array_has_a_case():
    driven = {("diffab_sample_loop_ex", "opt.ctx_of_row"): test_ctx_of_row_is_dead_on_return,
              ("diffab_sample_loop_ex", "opt.record.slot_of_step"): test_slot_of_step_is_dead_on_return,
              ("diffab_sample_loop_ex", "opt.steps.steps"): test_the_step_list_and_its_coefficients_are_dead_on_return,
              ("diffab_sample_loop_ex", "opt.steps.beta_jump"): test_the_step_list_and_its_coefficients_are_dead_on_return,
              ("diffab_sample_loop_ex", "opt.steps.alpha_jump"): test_the_step_list_and_its_coefficients_are_dead_on_return,
              ("diffab_score_designs", "ctx_of_design"): test_the_scorer_s_host_arrays_are_dead_on_return,
              ("diffab_score_designs", "t_list"): test_the_scorer_s_host_arrays_are_dead_on_return,
              ("diffab_metrics_pair_energy", "bin_edges"): test_bin_edges_are_dead_on_return,
              ("diffab_metrics_motifs", "motifs"): test_motifs_are_dead_on_return,
              ("diffab_metrics_surface", "point_radius"): test_point_radius_is_dead_on_return,
              ("diffab_patch_gather", "complex_of_row"): test_complex_of_row_is_dead_on_return}
    assert set(driven) == set(HOST_ARRAYS)


HOST_ARRAY_TESTS = test_every_host_array_has_a_case  # (tests/test_stream_contract_host.py runs it without a device)


# ---------------------------------------------------------------------------------------------------------------- 3. negative controls
class StandIn:
    """diffab_so3_log written in Python: S = R + 1 (as tests/test_operand_extents_host.py's).  how = "on_stream": the copy on the stream
    it is handed; "default_stream": on the caller's current stream instead; "synchronize": on its stream, after draining the device."""

    def __init__(self, how):
        self.how, self.abi, self.streams = how, None, []

    def _f32(self, p, n):
        p = int((p.value if isinstance(p, C.c_void_p) else p) or 0)
        for s in self.abi.last.values():
            base = s["buf"].data_ptr()
            if base <= p < base + s["buf"].numel():
                return s["buf"][p - base:p - base + 4 * n].view(torch.float32)
        raise KeyError(hex(p))

    def diffab_so3_log(self, R, S, n, stream):
        self.streams.append(int(stream.value or 0))
        src, dst = self._f32(R, 9 * n), self._f32(S, 9 * n)
        if self.how == "synchronize":
            torch.cuda.synchronize()
        if self.how == "default_stream":
            torch.add(src, 1.0, out=dst)
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream.value))):
                torch.add(src, 1.0, out=dst)
        return 0


def stand_in_call(how, n=1000):
    R = torch.randn(n, 3, 3, device="cuda")
    S = torch.full((n, 3, 3), 9.0, device="cuda")
    torch.add(torch.zeros(1, device="cuda"), 1.0)  # (the add kernel is loaded: the stand-in's host time is a launch)
    stand = StandIn(how)
    with GatedStreamABI(("diffab_so3_log",), lib=stand) as abi:
        stand.abi = abi
        rc = _hip.lib().diffab_so3_log(_hip.ptr(R), _hip.ptr(S), n, _hip.stream_ptr())
        seen = S.clone()  # (on the caller's stream, which waits for the harness: no host synchronisation needed)
    assert rc == 0 and stand.streams and all(s == abi.stream.cuda_stream for s in stand.streams)
    return abi, R, seen


def test_a_correct_stand_in_passes(hip):
    abi, R, S = stand_in_call("on_stream")
    assert torch.equal(S, R + 1) and abi.counts == {"diffab_so3_log": 2}
    assert [c[1] for c in abi.calls] == [True] and abi.calls[0][4] == 1


def test_a_copy_on_the_default_stream_is_reported_through_its_value(hip):
    """The stray kernel runs during the gate: it reads the decoy (R / 2), and what it wrote is overwritten by the copy-in of S."""
    abi, R, S = stand_in_call("default_stream")
    assert not torch.equal(S, R + 1)
    assert bool((S == 9.0).all()), "the caller's S came back as it went in: the stray result was overwritten"
    assert [c[1] for c in abi.calls] == [True]


def test_a_host_wait_inside_the_call_is_reported_as_waiting(hip):
    with pytest.raises(EntryWaited) as err:
        stand_in_call("synchronize")
    assert "diffab_so3_log held the host" in str(err.value)


# ---------------------------------------------------------------------------------------------------------------- 4. the other direction
def train_through_the_front_end():
    """(model, inputs, run): the K = 64 training step of tests/test_gpu_operand_alignment.py through hotpath_train_losses + backward."""
    from diffab_pytorch import DiffAb
    from test_gpu_operand_alignment import DIMS, train_case

    c = train_case(64)
    torch.manual_seed(0)
    model = DiffAb(DIMS["D"], DIMS["C"], DIMS["NL"], DIMS["DS"], DIMS["PQ"], DIMS["PV"], DIMS["H"]).cuda()
    model.denoiser.load_state_dict(c["sd"])
    inp = {k: v.cuda() for k, v in c["inp"].items()}
    nz = {k: v.cuda() for k, v in c["nz"].items()}
    beta = c["beta"].cuda()
    torch.cuda.synchronize()

    def run():
        rc = inp["res_context_emb"].clone().requires_grad_(True)
        pc = inp["pair_context_emb"].clone().requires_grad_(True)
        ls = model.hotpath_train_losses(nz, rc, pc, beta, inp["orientations"], inp["generation_mask"], inp["residue_mask"])
        (ls[0] + ls[1] + ls[2]).backward()
        return ls, rc, pc

    return c, model, run


def check_training_step(c, model, ls, rc, pc, what):
    from conftest import maxrel
    from sampler_support import GTOL, check_params

    np.testing.assert_allclose([float(v) for v in ls], c["losses"], rtol=5e-5)
    r_rc, r_pc = maxrel(rc.grad, c["d_rc"]), maxrel(pc.grad, c["d_pc"])
    assert r_rc < GTOL and r_pc < GTOL, (what, r_rc, r_pc)
    check_params(model.denoiser.named_parameters(), c["sdo"], "denoiser.", what)


def test_training_step_behind_the_gate_with_the_stream_guard_on(hip):
    """diffab_set_stream_guard(1): before a call enqueues on another stream than the library's last, what it enqueued there is ordered
    in front by an event - never by a host wait.  The training step at K = 64, gated, against the float64 oracle."""
    c, model, run = train_through_the_front_end()
    assert hip.diffab_set_stream_guard(1) == 0
    try:
        with GatedStreamABI(TRAIN, known=tensors_of(model), gate=GATE) as abi:
            ls, rc, pc = run()
        report("stream guard on", abi)
    finally:
        assert hip.diffab_set_stream_guard(0) == 0
    assert all(abi.counts.get(e, 0) > 0 for e in TRAIN), abi.counts
    assert_returned_early("stream guard on", abi)
    check_training_step(c, model, ls, rc, pc, "training step behind the gate, stream guard on")


def test_nothing_is_ordered_behind_the_default_stream(hip):
    """The caller's current stream is a side stream of its own and the legacy default stream is busy for two seconds: the gated training
    step (the backward forks an internal stream, SideRun of csrc/denoiser_backward.hip) is finished when the caller's stream is, while
    the default stream is still busy - nothing of it waits for stream 0 - and equals the float64 oracle."""
    c, model, run = train_through_the_front_end()
    _, cycles_per_ms = gated_stream()
    caller = torch.cuda.Stream()
    busy, finished = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    torch.cuda._sleep(int(2000 * cycles_per_ms))  # (bounded device work on stream 0)
    busy.record(torch.cuda.default_stream())
    t0 = time.perf_counter()
    with torch.cuda.stream(caller):  # (the inputs were synchronised above: the caller's stream itself waits for nothing on stream 0)
        with GatedStreamABI(TRAIN, known=tensors_of(model), gate=GATE) as abi:
            ls, rc, pc = run()
            finished.record(caller)
            finished.synchronize()
            default_still_busy = not busy.query()
    seconds = time.perf_counter() - t0
    report("default stream busy", abi)
    torch.cuda.synchronize()
    assert default_still_busy, ("the training step was ordered behind the default stream", seconds)
    assert all(abi.counts.get(e, 0) > 0 for e in TRAIN), abi.counts
    check_training_step(c, model, ls, rc, pc, "training step on a side stream, default stream busy")
