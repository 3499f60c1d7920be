"""Design novelty on the MI355X: metrics.novelty / diffab_metrics_edit_nearest and metrics.design_sequences /
diffab_metrics_pack_sequences against the numpy restatement of novelty_ref.py (the plain dynamic programme), their properties and
their contracts.

Everything is compared BIT FOR BIT: the distances, indices and counts are integers, and identity is one correctly rounded fp32
division and one subtraction of integers below 2^9.  No tolerance exists.  The restatement's own hand-made cases are in
tests/test_novelty_host.py.  R * M of a case stays at or below about 20 000 so that the dynamic programme takes seconds."""
import functools

import numpy as np
import pytest
import torch

import sampler_support
from diffab_pytorch import _hip, metrics
from novelty_ref import PAD, PER_QUERY, edit_matrix, nearest_ref, pack_ref, same_bits
from sampler_support import GuardedABI, header_prototypes, hip, misaligned
from scratch_poison import poisoned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
numpy_of = lambda out: {k: v.cpu().numpy() for k, v in out.items()}
OUTPUTS = ("distance", "index", "n_within", "identity", "matrix")
Q_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64)
LIB_LENGTHS = (0, 1, 17, 64, 65, 200, 256)


# ------------------------------------------------------------------ inputs
def sequences(rng, lengths, width, alphabet, behind=PAD):
    """(tokens (n, width) uint8, lengths (n) int32): random tokens below `alphabet`, `behind` (a value, or "random") past each length."""
    lengths = np.asarray(lengths, np.int32)
    tokens = rng.integers(0, alphabet, (len(lengths), width)).astype(np.uint8)
    past = np.arange(width)[None, :] >= np.clip(lengths, 0, width)[:, None]
    tokens[past] = rng.integers(0, alphabet, int(past.sum())).astype(np.uint8) if behind == "random" else behind
    return tokens, lengths


def edited(rng, seq, n_edits, alphabet, limit):
    """`seq` (a list of tokens) after n_edits random insertions, deletions and substitutions, at most `limit` long."""
    s = list(seq)
    for _ in range(n_edits):
        kind = rng.integers(0, 3)
        if kind == 0 and len(s) < limit:
            s.insert(int(rng.integers(0, len(s) + 1)), int(rng.integers(0, alphabet)))
        elif kind == 1 and s:
            del s[int(rng.integers(0, len(s)))]
        elif s:
            s[int(rng.integers(0, len(s)))] = int(rng.integers(0, alphabet))
    return s


def plant(rng, q, nq, lib, nl, alphabet):
    """A third of the library replaced by queries after 0 - 3 edits, at random places; the queries take turns."""
    LM = lib.shape[1]
    for k, m in enumerate(rng.choice(len(lib), max(1, len(lib) // 3), replace=False)):
        r = k % len(q)
        s = edited(rng, q[r, :nq[r]].tolist(), int(rng.integers(0, 4)), alphabet, LM)
        lib[m], nl[m] = PAD, len(s)
        lib[m, :len(s)] = s


def sets_of(q, nq, lib, nl):
    return metrics.SequenceSet(cuda(q), cuda(nq)), metrics.SequenceSet(cuda(lib), cuda(nl))


def device(q, nq, lib, nl, radius=None, exclude=None, matrix=True):
    """metrics.novelty on the device, its outputs as numpy with index as the int32 the entry writes."""
    exclude = cuda(np.asarray(exclude, np.int64)) if exclude is not None and not isinstance(exclude, str) else exclude
    out = numpy_of(metrics.novelty(*sets_of(q, nq, lib, nl), radius=radius, exclude=exclude, matrix=matrix))
    assert out["index"].dtype == np.int64
    out["index"] = out["index"].astype(np.int32)
    return out


def check(got, want, what, only=OUTPUTS):
    for k in only:
        if k in got:
            assert same_bits(got[k], want[k]), (what, k, got[k], want[k])
    if "length" in got:
        assert got["length"].dtype == np.int32 and got["nearest_length"].dtype == np.int32


def compare(q, nq, lib, nl, what, radius=3, skip=None, matrix=None):
    """The device against the restatement (`matrix`: the restatement's distances where a test has them already)."""
    want = nearest_ref(q, nq, lib, nl, skip=skip, radius=-1 if radius is None else radius, matrix=matrix)
    got = device(q, nq, lib, nl, radius=radius, exclude=skip)
    assert ("n_within" in got) == (radius is not None)
    check(got, want, what)
    derived = nearest_ref(q, nq, lib, nl, skip=skip, radius=-1 if radius is None else radius, matrix=got["matrix"])
    check(got, derived, what + " (from the device matrix)", only=PER_QUERY)  # the four per-query outputs are what the matrix implies
    LQ, LM = q.shape[1], lib.shape[1]
    assert np.array_equal(got["length"], np.clip(nq, 0, LQ))
    near = np.where(want["index"] >= 0, np.clip(nl, 0, LM)[np.maximum(want["index"], 0)] if len(nl) else -1, -1)
    assert np.array_equal(got["nearest_length"], near), what
    return got, want


@functools.lru_cache(maxsize=None)
def length_case(alphabet, planted):
    rng = np.random.default_rng(100 * alphabet + planted)
    q, nq = sequences(rng, list(Q_LENGTHS) * 2, 64, alphabet)
    lib, nl = sequences(rng, list(LIB_LENGTHS) * 10, 256, alphabet)
    if planted:
        plant(rng, q, nq, lib, nl, alphabet)
    return q, nq, lib, nl


@functools.lru_cache(maxsize=None)
def length_matrix(alphabet, planted):
    """The restatement's distances of length_case, computed once."""
    return edit_matrix(*length_case(alphabet, planted))


# ------------------------------------------------------------------ (a) against the restatement
@pytest.mark.parametrize("planted", [False, True], ids=["random", "planted"])
@pytest.mark.parametrize("alphabet", [2, 3, 21])
def test_every_length_equals_the_restatement_bit_for_bit(alphabet, planted):
    q, nq, lib, nl = length_case(alphabet, planted)
    got, want = compare(q, nq, lib, nl, f"alphabet {alphabet} planted {planted}", matrix=length_matrix(alphabet, planted))
    assert set(nq) == set(Q_LENGTHS) and set(LIB_LENGTHS) <= set(nl)
    if planted:
        assert (want["distance"] <= 3).all() and (want["n_within"] > 0).all() and (want["distance"] == 0).any()
    else:
        assert want["distance"].max() > 3


def test_carries_from_bit_31_into_bit_32():
    """A run of matches is a carry chain through the whole word: a 64-long query of one letter against texts of that letter, and
    queries that match in one half of the word only.  The answers are counted by hand: a text token that finds no partner costs one,
    and so does a query token."""
    A, R = 0, 1
    one = lambda s: (np.array([s + [PAD] * (64 - len(s))], np.uint8), np.array([len(s)], np.int32))
    texts = [[A] * n for n in (1, 32, 33, 64, 65)] + [[A] * 32 + [R] * 32, [R] * 32 + [A] * 32, [A] * 31 + [R] + [A] * 32, [A] * 64 + [R] * 64]
    lib = np.full((len(texts), 131), PAD, np.uint8)
    for m, t in enumerate(texts):
        lib[m, :len(t)] = t
    nl = np.array([len(t) for t in texts], np.int32)
    for name, query, answer in (("all one letter", [A] * 64, [63, 32, 31, 0, 1, 32, 32, 1, 64]),
                                ("positions 0 - 31 match", [A] * 32 + [R] * 32, [63, 32, 32, 32, 33, 0, 64, 33, 64]),
                                ("positions 32 - 63 match", [R] * 32 + [A] * 32, [63, 32, 32, 32, 33, 64, 0, 31, 96]),
                                ("33 of one letter", [A] * 33, [32, 1, 0, 31, 32, 32, 32, 31, 95])):
        q, nq = one(query)
        got, want = compare(q, nq, lib, nl, name, radius=32)
        assert got["matrix"][0].tolist() == answer and want["matrix"][0].tolist() == answer, (name, got["matrix"][0].tolist())


EXTENTS = [(1, 1), (65, 1), (65, 63), (63, 64), (63, 65), (20, 1000), (1, 4097), (4, 4097)]


@pytest.mark.parametrize("R, M", EXTENTS)
def test_extents_and_row_strides_that_are_no_multiple_of_four(R, M):
    """More than one tile of queries, more than one pass, wave and chunk of entries, rows of 23 and 37 bytes."""
    rng = np.random.default_rng(7 * R + M)
    q, nq = sequences(rng, rng.integers(0, 24, R), 23, 5)
    lib, nl = sequences(rng, rng.integers(0, 38, M), 37, 5)
    plant(rng, q, nq, lib, nl, 5)
    compare(q, nq, lib, nl, f"R={R} M={M}", radius=4, skip=rng.integers(-1, M + 1, R))


def test_ties_go_to_the_lower_index_across_lanes_waves_passes_and_chunks():
    rng = np.random.default_rng(11)
    M, places = 4097, [5, 6, 70, 300, 2047, 2048, 4096]
    q, nq = sequences(rng, [12, 12, 0], 16, 4)
    lib, nl = sequences(rng, rng.integers(14, 20, M), 19, 4)  # (nothing random comes near: the lengths alone cost 2)
    for m in places:
        lib[m], nl[m] = PAD, 12
        lib[m, :12] = q[0, :12]
    lib[4000, :] = PAD
    nl[4000] = nl[100] = 0  # the empty query's nearest: two empty entries
    for k, m in enumerate(places):
        skip = np.array([m, -1, 100])
        got, want = compare(q, nq, lib, nl, f"skip {m}", radius=0, skip=skip)
        assert got["index"].tolist()[0] == (places[0] if k else places[1]) and got["distance"].tolist() == [0, want["distance"][1], 0]
        assert got["n_within"].tolist() == [len(places) - 1, 0, 1] and got["index"][2] == 4000
    got, _ = compare(q, nq, lib, nl, "no skip", radius=0)
    assert got["index"].tolist()[0] == 5 and got["index"][2] == 100 and got["n_within"].tolist() == [len(places), 0, 2]


def test_skip_radius_and_exclude_self():
    q, nq, lib, nl = length_case(3, True)
    R, M = len(q), len(lib)
    base = nearest_ref(q, nq, lib, nl, matrix=length_matrix(3, True))
    for name, skip in (("in range", base["index"]), ("-1 and >= M", np.array([-1, M, M + 5, 2 ** 31 - 1] * 4)), ("mixed", np.where(np.arange(R) % 2, base["index"], -1))):
        for radius in (0, 3, 1000, None, -1):
            got, want = compare(q, nq, lib, nl, f"skip {name} radius {radius}", radius=radius, skip=skip, matrix=base["matrix"])
            if radius == 1000:
                assert (got["n_within"] == M - ((skip >= 0) & (skip < M))).all()
            if radius == -1:
                assert (got["n_within"] == 0).all()
    assert (nearest_ref(q, nq, lib, nl, skip=base["index"], matrix=base["matrix"])["index"] != base["index"]).all()
    # the set against itself
    both = np.full((R, 256), PAD, np.uint8)
    both[:, :64] = q
    want = nearest_ref(q, nq, both, nq, skip=np.arange(R), radius=0)
    got = device(q, nq, both, nq, radius=0, exclude="self")
    check(got, want, "exclude='self'")
    assert (got["matrix"].diagonal() == 0).all() and (got["index"] != np.arange(R)).all()
    assert (got["n_within"] == (want["matrix"] == 0).sum(1) - 1).all() and got["n_within"].any()  # (every length twice: the two empty queries)


def test_nothing_to_compare():
    q, nq, lib, nl = length_case(21, False)
    got = device(q, nq, lib[:0], nl[:0], radius=5)
    R = len(q)
    assert got["distance"].tolist() == [-1] * R and got["index"].tolist() == [-1] * R and got["n_within"].tolist() == [0] * R
    assert np.isnan(got["identity"]).all() and got["matrix"].shape == (R, 0) and got["nearest_length"].tolist() == [-1] * R
    check(got, nearest_ref(q, nq, lib[:0], nl[:0], radius=5), "M = 0")
    skip = np.array([0, -1, 1] + [0] * (R - 3))
    got, want = compare(q, nq, lib[3:4], nl[3:4], "one entry, skipped", radius=300, skip=skip)
    assert got["distance"][0] == -1 and got["distance"][1] >= 0 and np.isnan(got["identity"][0]) and got["n_within"].tolist()[:3] == [0, 1, 1]
    none = metrics.novelty(metrics.SequenceSet(cuda(q[:0]), cuda(nq[:0])), metrics.SequenceSet(cuda(lib), cuda(nl)), radius=1, matrix=True)
    assert tuple(none["distance"].shape) == (0,) and tuple(none["matrix"].shape) == (0, len(lib)) and none["index"].dtype == torch.int64


# ------------------------------------------------------------------ (b) properties
def test_the_distance_is_symmetric_with_the_roles_swapped():
    rng = np.random.default_rng(3)
    a, na = sequences(rng, list(Q_LENGTHS) * 3, 64, 3)
    b, nb = sequences(rng, rng.choice(Q_LENGTHS, 70), 64, 3)
    ab, ba = device(a, na, b, nb)["matrix"], device(b, nb, a, na)["matrix"]
    assert np.array_equal(ab, ba.T) and np.array_equal(ab, edit_matrix(a, na, b, nb))


def test_a_library_split_in_two_combines_to_the_whole():
    q, nq, lib, nl = length_case(3, True)
    rng = np.random.default_rng(5)
    lib, nl = np.concatenate([lib] * 31), np.concatenate([nl] * 31)  # 2170 entries: the whole has two chunks, the cut is inside the first
    order = rng.permutation(len(lib))
    lib, nl, cut = lib[order], nl[order], 1001
    distances = length_matrix(3, True)[:, order % 70]  # (entry m of the long library is entry order[m] % 70 of the short one)
    R = len(q)
    skip = rng.integers(0, len(lib), R)
    whole = device(q, nq, lib, nl, radius=2, exclude=skip)
    lo = device(q, nq, lib[:cut], nl[:cut], radius=2, exclude=skip)
    hi = device(q, nq, lib[cut:], nl[cut:], radius=2, exclude=skip - cut)
    assert np.array_equal(whole["matrix"], np.concatenate([lo["matrix"], hi["matrix"]], 1)) and np.array_equal(whole["matrix"], distances)
    assert np.array_equal(whole["n_within"], lo["n_within"] + hi["n_within"])
    first = (lo["distance"] >= 0) & ((hi["distance"] < 0) | (lo["distance"] <= hi["distance"]))
    assert np.array_equal(whole["distance"], np.where(first, lo["distance"], hi["distance"]))
    assert np.array_equal(whole["index"], np.where(first, lo["index"], hi["index"] + cut))
    assert same_bits(whole["identity"], np.where(first, lo["identity"], hi["identity"]))
    check(whole, nearest_ref(q, nq, lib, nl, skip=skip, radius=2, matrix=whole["matrix"]), "whole", only=PER_QUERY)


def test_a_query_alone_gives_the_bits_it_gives_among_others():
    q, nq, lib, nl = length_case(21, True)
    among = device(q, nq, lib, nl, radius=3)
    check(among, nearest_ref(q, nq, lib, nl, radius=3, matrix=length_matrix(21, True)), "among others")
    for r in (0, 5, 15):
        alone = device(q[r:r + 1], nq[r:r + 1], lib, nl, radius=3)
        for k in OUTPUTS:
            assert same_bits(alone[k], among[k][r:r + 1]), (r, k)
    narrow = device(q[:3, :2], nq[:3], lib, nl, radius=3)  # queries of lengths 0, 1, 2 in rows of two bytes
    for k in OUTPUTS:
        assert same_bits(narrow[k], among[k][:3]), k


def test_tokens_of_32_or_more_match_nothing_and_bytes_behind_the_length_change_nothing():
    rng = np.random.default_rng(9)
    q, nq = sequences(rng, rng.integers(0, 41, 24), 40, 4)
    lib, nl = sequences(rng, rng.integers(0, 51, 90), 50, 4)
    plant(rng, q, nq, lib, nl, 4)
    for t, n in ((q, nq), (lib, nl)):  # high tokens on either side, the same ones on both: 31 matches, 32, 40, 200 and 255 do not
        inside = np.arange(t.shape[1])[None, :] < n[:, None]
        hit = inside & (rng.random(t.shape) < 0.3)
        t[hit] = rng.choice([31, 32, 40, 200, 255], int(hit.sum())).astype(np.uint8)
    got, want = compare(q, nq, lib, nl, "high tokens", radius=5)
    assert (want["matrix"][(nq > 0)] > 0).any()
    plain = lambda t: np.where(t >= 32, 33, t)  # every such token is as good as any other that matches nothing
    assert np.array_equal(got["matrix"], edit_matrix(plain(q), nq, plain(lib), nl))
    # bytes behind the lengths: letters that would match
    rng = np.random.default_rng(10)
    q2, lib2 = q.copy(), lib.copy()
    q2[np.arange(q.shape[1])[None, :] >= nq[:, None]] = 1
    lib2[np.arange(lib.shape[1])[None, :] >= nl[:, None]] = 1
    filled = device(q2, nq, lib2, nl, radius=5)
    for k in OUTPUTS:
        assert same_bits(filled[k], got[k]), k
    # lengths outside their rows are read as clamped
    wild_q = np.where(np.arange(len(nq)) % 3 == 0, nq + 1000, nq).astype(np.int32)
    wild_q[1], wild_q[2] = -7, -2 ** 31
    wild_l = np.where(np.arange(len(nl)) % 4 == 0, 2 ** 31 - 1, nl).astype(np.int32)
    wild_l[1], wild_l[2] = -1, 51
    wild = device(q2, wild_q, lib2, wild_l, radius=5)
    clamped = device(q2, np.clip(wild_q, 0, 40), lib2, np.clip(wild_l, 0, 50), radius=5)
    for k in OUTPUTS + ("length", "nearest_length"):
        assert same_bits(wild[k], clamped[k]), k
    check(wild, nearest_ref(q2, wild_q, lib2, wild_l, radius=5), "clamped lengths")


# ------------------------------------------------------------------ (c) design rows as sequences
def pack_case(K, N=3, G=2, seed=0):
    rng = np.random.default_rng(K + seed)
    tokens = rng.integers(0, 21, (G * N, K))
    odd = rng.random(tokens.shape) < 0.2
    tokens[odd] = rng.choice([-1, 254, 255, 300, 31, 32], int(odd.sum()))
    mask = rng.random((G, K)) < 0.4
    mask[:, [0, K - 1]] = True
    if K > 64:
        mask[:, 62:67] = True  # counted slots on both sides of slot 64
    rm = rng.random((G, K)) < 0.8
    seg = rng.integers(0, 3, (G, K))
    return tokens, mask, rm, seg


def raw_pack(tokens, mask, rm, seg, segment, group_size, L, shifted=False, skip=()):
    place = lambda t: misaligned(t, 4 if t.element_size() >= 4 else 3) if shifted else t
    rows, K = tokens.shape
    ops = [cuda(tokens.astype(np.int32)), cuda(mask), None if rm is None else cuda(rm), None if seg is None else cuda(seg.astype(np.int32))]
    ops = [None if t is None else place(t) for t in ops]
    out = {"out_tokens": place(torch.empty(rows, L, dtype=torch.uint8, device="cuda")), "out_len": place(torch.empty(rows, dtype=torch.int32, device="cuda"))}
    out = {k: v for k, v in out.items() if k not in skip}
    lib = _hip.lib()
    rc = lib.diffab_metrics_pack_sequences(*[_hip.ptr(t) for t in ops], segment, rows, group_size, K, L, _hip.ptr(out.get("out_tokens")),
                                           _hip.ptr(out.get("out_len")), _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


@pytest.mark.parametrize("K", [1, 64, 65, 130])
def test_pack_sequences_equals_a_gather(K):
    tokens, mask, rm, seg = pack_case(K)
    for rm_, seg_, segment, L in ((None, None, 0, 256), (rm, None, 0, 64), (rm, seg, 2, 64), (None, seg, 1, 7), (None, None, 0, 1)):
        want_t, want_n = pack_ref(tokens, mask, rm_, seg_, segment, 3, L)
        got = raw_pack(tokens, mask, rm_, seg_, segment, 3, L)
        assert same_bits(got["out_tokens"], want_t) and same_bits(got["out_len"], want_n), (K, L, segment)
    if K == 130:
        assert (want_n > 1).any() and (pack_ref(tokens, mask, None, seg, 1, 3, 7)[1] > 7).any()  # a count above L: reported, the tokens cut
        assert {255} < set(pack_ref(tokens, mask, None, None, 0, 3, 256)[0][:, :20].flatten().tolist())
    only_len = raw_pack(tokens, mask, rm, seg, 2, 3, 64, skip=("out_tokens",))
    assert set(only_len) == {"out_len"} and same_bits(only_len["out_len"], pack_ref(tokens, mask, rm, seg, 2, 3, 64)[1])
    only_tok = raw_pack(tokens, mask, rm, seg, 2, 3, 64, skip=("out_len",))
    assert same_bits(only_tok["out_tokens"], pack_ref(tokens, mask, rm, seg, 2, 3, 64)[0])


def test_design_sequences_and_its_refusal_of_a_long_patch():
    tokens, mask, rm, seg = pack_case(130)
    designs = {"seq_idx": cuda(tokens)}
    s = metrics.design_sequences(designs, cuda(mask), group_size=3, residue_mask=cuda(rm), segment_idx=cuda(seg), segment=2, max_length=64)
    want_t, want_n = pack_ref(tokens, mask, rm, seg, 2, 3, 64)
    assert s.tokens.is_cuda and same_bits(s.tokens.cpu().numpy(), want_t) and same_bits(s.lengths.cpu().numpy(), want_n)
    strings = metrics.sequence_strings(s)
    assert [len(x) for x in strings] == want_n.tolist() and "?" in "".join(strings)
    n = int((mask & rm).sum(1).max())
    with pytest.raises(ValueError, match=rf"has {n} counted residues, more than max_length = {n - 1}"):
        metrics.design_sequences(designs, cuda(mask), group_size=3, residue_mask=cuda(rm), max_length=n - 1)
    on_cpu = metrics.design_sequences({"seq_idx": torch.from_numpy(tokens)}, torch.from_numpy(mask), group_size=3, max_length=256)
    assert not on_cpu.tokens.is_cuda and same_bits(on_cpu.tokens.numpy(), pack_ref(tokens, mask, None, None, 0, 3, 256)[0])


# ------------------------------------------------------------------ (d) contracts
def raw_nearest(q, nq, lib, nl, skip=None, radius=3, leave=(), shifted=False):
    """diffab_metrics_edit_nearest on device operands, through whatever stands in for _hip.lib()."""
    place = lambda t: misaligned(t, 4 if t.element_size() >= 4 else 3) if shifted else t
    (R, LQ), (M, LM) = q.shape, lib.shape
    ops = [cuda(q), cuda(nq.astype(np.int32)), cuda(lib), cuda(nl.astype(np.int32)), None if skip is None else cuda(np.asarray(skip, np.int32))]
    ops = [None if t is None else place(t) for t in ops]
    shapes = {"distance": (R,), "index": (R,), "n_within": (R,), "identity": (R,), "matrix": (R, M)}
    out = {k: place(torch.empty(s, dtype=torch.float32 if k == "identity" else torch.int32, device="cuda")) for k, s in shapes.items() if k not in leave}
    nbytes = metrics.edit_nearest_workspace_bytes(R, M, LM)
    ws = _hip.workspace(nbytes)
    lib_ = _hip.lib()
    rc = lib_.diffab_metrics_edit_nearest(_hip.ptr(ops[0]), _hip.ptr(ops[1]), R, LQ, _hip.ptr(ops[2]), _hip.ptr(ops[3]), M, LM, _hip.ptr(ops[4]), radius,
                                          *[_hip.ptr(out.get(k)) for k in OUTPUTS], _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


@functools.lru_cache(maxsize=None)
def contract_case(R=33, M=2100, LQ=23, LM=37):
    rng = np.random.default_rng(R + M)
    q, nq = sequences(rng, rng.integers(0, LQ + 1, R), LQ, 4, behind="random")
    lib, nl = sequences(rng, rng.integers(0, LM + 1, M), LM, 4, behind="random")
    plant(rng, q, nq, lib, nl, 4)
    skip = rng.integers(-1, M, R)
    return q, nq, lib, nl, skip, nearest_ref(q, nq, lib, nl, skip=skip, radius=3)


@pytest.mark.parametrize("leave", [("matrix",), ("distance",), ("index", "n_within"), ("identity", "matrix"), OUTPUTS[:4], OUTPUTS])
def test_null_outputs_are_skipped_and_the_others_unchanged(leave):
    q, nq, lib, nl, skip, want = contract_case()
    got = raw_nearest(q, nq, lib, nl, skip, leave=leave)
    assert set(got) == set(OUTPUTS) - set(leave)
    check(got, want, f"without {leave}")


@pytest.mark.parametrize("fill", ["ff", "random"])
def test_what_the_workspace_and_the_outputs_held_is_ignored(fill):
    q, nq, lib, nl, skip, want = contract_case()
    with poisoned(fill, seed=5):
        check(device(q, nq, lib, nl, radius=3, exclude=skip), want, f"under {fill}")
        check(raw_nearest(q, nq, lib, nl, skip, leave=("matrix",)), want, f"four outputs under {fill}")
        check(raw_nearest(q, nq, lib, nl, skip, leave=OUTPUTS[:4]), want, f"the matrix under {fill}")
        small = contract_case(5, 3, 64, 256)
        check(raw_nearest(*small[:5]), small[5], f"three entries under {fill}")
        tokens, mask, rm, seg = pack_case(130)
        s = metrics.design_sequences({"seq_idx": cuda(tokens)}, cuda(mask), group_size=3, residue_mask=cuda(rm), max_length=100)
        want_t, want_n = pack_ref(tokens, mask, rm, None, 0, 3, 100)
        assert same_bits(s.tokens.cpu().numpy(), want_t) and same_bits(s.lengths.cpu().numpy(), want_n)


NOVELTY_ARGTYPES = {n: a for n, (_, a) in _hip.NOVELTY_SYMBOLS.items()}
NOVELTY_WRITES = {"diffab_metrics_edit_nearest": " ".join(OUTPUTS) + " workspace", "diffab_metrics_pack_sequences": "out_tokens out_len"}


@pytest.mark.parametrize("fill", sampler_support.GUARD_FILLS)
def test_outputs_between_guards_with_operands_at_their_natural_alignment(fill, monkeypatch):
    for entry, writes in NOVELTY_WRITES.items():
        monkeypatch.setitem(sampler_support.WRITES, entry, writes)
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes(("diffab_hip_novelty.h",))[1].items()}
    assert set(params) == set(NOVELTY_ARGTYPES)
    with GuardedABI(tuple(NOVELTY_ARGTYPES), fill, argtypes=NOVELTY_ARGTYPES) as abi:
        abi.params.update(params)
        for shape in ((33, 2100, 23, 37), (5, 3, 64, 256), (17, 65, 1, 1)):
            q, nq, lib, nl, skip, want = contract_case(*shape)
            check(raw_nearest(q, nq, lib, nl, skip, shifted=True), want, f"{shape} guarded [{fill}]")
        q, nq, lib, nl, skip, want = contract_case()
        check(raw_nearest(q, nq, lib, nl, None, leave=OUTPUTS[:4], shifted=True), nearest_ref(q, nq, lib, nl, radius=3), "guarded, the matrix alone")
        for K in (1, 65, 130):
            tokens, mask, rm, seg = pack_case(K)
            got = raw_pack(tokens, mask, rm, seg, 1, 3, 9, shifted=True)
            want_t, want_n = pack_ref(tokens, mask, rm, seg, 1, 3, 9)
            assert same_bits(got["out_tokens"], want_t) and same_bits(got["out_len"], want_n), K
    assert abi.counts["diffab_metrics_edit_nearest"] >= 3 * 10 and abi.counts["diffab_metrics_pack_sequences"] >= 3 * 6


# ------------------------------------------------------------------ (e) end to end
def test_sampled_designs_against_a_library_that_holds_them():
    """sample(num_samples = 4) of the unit model at K = 64 -> design_sequences -> novelty against a library that holds every design once
    among decoys: each design finds itself at distance 0, and with that entry excluded what the restatement says."""
    dims, model, _ = sampler_support.unit_model()
    G, K, N = 2, 64, 4
    inp = sampler_support.patches(G, K, dims, seed=5)
    res = sampler_support.sample(model, inp, seed=3, num_samples=N, steps=2)
    gm = inp["generation_mask"]
    designs = metrics.design_sequences(res, gm, group_size=N)
    rows = G * N
    want_t, want_n = pack_ref(res["seq_idx"].cpu().numpy(), gm.cpu().numpy(), group_size=N, L=64)
    q, nq = designs.tokens.cpu().numpy(), designs.lengths.cpu().numpy()
    assert same_bits(q, want_t) and same_bits(nq, want_n) and (nq > 0).all() and tuple(q.shape) == (rows, 64)
    rng = np.random.default_rng(2)
    M = 300
    lib, nl = sequences(rng, rng.integers(3, 30, M), 70, 21)
    own = rng.choice(M, rows, replace=False)  # where each design's own copy goes; no design is put in twice
    for r, m in enumerate(own):
        lib[m], nl[m] = PAD, nq[r]
        lib[m, :nq[r]] = q[r, :nq[r]]
    library = metrics.SequenceSet(cuda(lib), cuda(nl))
    out = numpy_of(metrics.novelty(designs, library, radius=0))
    first = nearest_ref(q, nq, lib, nl, radius=0)
    assert (out["distance"] == 0).all() and (out["identity"] == 1).all() and np.array_equal(out["index"], first["index"])
    same = (first["matrix"][:, own] == 0)  # (two designs of a patch may be the same sequence: then the lower entry is the nearest)
    assert np.array_equal(out["index"], np.array([own[same[r]].min() for r in range(rows)])) and np.array_equal(out["n_within"], same.sum(1))
    out = numpy_of(metrics.novelty(designs, library, radius=2, exclude=cuda(own), matrix=True))
    out["index"] = out["index"].astype(np.int32)
    check(out, nearest_ref(q, nq, lib, nl, skip=own, radius=2), "own entry excluded")
    assert (out["index"] != own).all()
    # the designs of patch 0 against themselves, as a distance matrix for cluster
    mine = metrics.SequenceSet(designs.tokens[:N], designs.lengths[:N])
    dist = metrics.novelty(mine, mine, matrix=True)["matrix"]
    clusters = metrics.cluster(dist.float().view(1, N, N), 0.5)
    assert tuple(clusters["label"].shape) == (1, N) and (dist.diagonal() == 0).all() and torch.equal(dist, dist.T)
