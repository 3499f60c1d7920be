"""CPU: the host side of patch construction from a whole complex (diffab_pytorch.patch, io.read_pdb, io.chothia_cdr_mask) - the numpy
restatement of the selection on a hand case, the C-ABI entries and their host-side refusals, the argument checks that happen before any
library call, and the PDB reader.

The rule is DESIGN.md section 4.12 / include/diffab_hip.h (diffab_patch_select, diffab_patch_gather, diffab_patch_scatter)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from diffab_pytorch import DiffAb, _hip, io as dio, patch
from sampler_support import ReachedTheLibrary, refuse_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement (shared with test_gpu_patch.py)
def select_ref(ca, gen, k, k_antigen=0, K=None, residue_mask=None, anchor_mask=None, chain=None, antigen=None, dtype=np.float64):
    """The four-step definition for ONE complex: ca (N,3), masks (N,).  Returns (index (K,), mask (K,), count, gaps): gaps = the relative
    gap (key[k+1] - key[k]) / key[k+1] between the keys at ranks k and k+1 of the all-residue pass and of the antigen pass (inf where
    there is no rank k+1, or rank k is a forced residue and rank k+1 is not)."""
    ca = np.asarray(ca, dtype)
    N = ca.shape[0]
    K = k + k_antigen if K is None else K
    present = np.ones(N, bool) if residue_mask is None else np.asarray(residue_mask, bool)
    gen = np.asarray(gen, bool) & present
    chain = np.zeros(N, np.int64) if chain is None else np.asarray(chain)
    empty = (np.full(K, -1, np.int64), np.zeros(K, bool))
    if not gen.any():
        return (*empty, 0, (np.inf, np.inf))
    if anchor_mask is None:  # 1. the residues flanking each generated segment on its chain
        anchors = np.zeros(N, bool)
        for i in range(N):
            left = i > 0 and gen[i - 1] and chain[i - 1] == chain[i]
            right = i < N - 1 and gen[i + 1] and chain[i + 1] == chain[i]
            anchors[i] = present[i] and not gen[i] and (left or right)
    else:
        anchors = np.asarray(anchor_mask, bool) & present
    if not anchors.any():
        anchors = gen.copy()
    forced = gen | anchors
    if forced.sum() > k:
        return (*empty, -1, (np.inf, np.inf))
    a = ca[anchors]
    dx, dy, dz = (ca[:, None, c] - a[None, :, c] for c in range(3))
    key = ((dx * dx + dy * dy) + dz * dz).min(1)  # 2. in exactly this association
    key[forced] = -1
    order = [i for i in np.lexsort((np.arange(N), key)) if present[i]]  # 3. (key, index) ascending
    s1 = order[:k]
    ag_order = [] if antigen is None or k_antigen == 0 else [i for i in order if np.asarray(antigen, bool)[i]]
    s2 = ag_order[:k_antigen]

    def gap(seq, n):
        if n == 0 or len(seq) <= n:
            return np.inf
        lo, hi = float(key[seq[n - 1]]), float(key[seq[n]])
        return np.inf if lo < 0 <= hi else (0.0 if hi == lo else (hi - lo) / hi)

    sel = sorted(set(s1) | set(s2))  # 4. ascending residue index
    index = np.full(K, -1, np.int64)
    index[:len(sel)] = sel
    return index, np.arange(K) < len(sel), len(sel), (gap(order, k), gap(ag_order, k_antigen))


def hand_case():
    """12 residues: an antibody chain 0-7 with generated residues 3, 4 (anchors 2 and 5), an antigen chain 8-11.  Keys (squared distance
    to the nearer of the anchors at x = 0 and x = 3): residue 0: 36, 1: 4, 6: 4, 7: 36, 8: 1, 9: 25, 10: 49, 11: 289."""
    ca = np.zeros((12, 3))
    ca[:8, 0] = [-6, -2, 0, 1, 2, 3, 5, 9]
    ca[8:] = [[0, 1, 0], [3, 5, 0], [10, 0, 0], [20, 0, 0]]
    gen = np.zeros(12, bool)
    gen[3:5] = True
    chain = np.array([1] * 8 + [3] * 4)
    return ca, gen, chain, chain == 3


def test_oracle_on_the_hand_case():
    ca, gen, chain, antigen = hand_case()
    # k = 6: the forced residues 2, 3, 4, 5, then residue 8 (key 1), then residue 1 - its key 4 ties with residue 6, the lower index wins.
    # k_antigen = 2: the antigen residues 8 (key 1) and 9 (key 25).  The union has 7 residues.
    index, mask, count, gaps = select_ref(ca, gen, 6, 2, 8, chain=chain, antigen=antigen)
    assert index.tolist() == [1, 2, 3, 4, 5, 8, 9, -1] and mask.tolist() == [True] * 7 + [False] and count == 7
    assert gaps[0] == 0.0 and gaps[1] == pytest.approx((49 - 25) / 49)
    # residue 8 absent: ranks 5 and 6 are the tied residues 1 and 6; the antigen pass takes 9 and 10
    rm = np.ones(12, bool)
    rm[8] = False
    index, mask, count, _ = select_ref(ca, gen, 6, 2, 8, residue_mask=rm, chain=chain, antigen=antigen)
    assert index.tolist() == [1, 2, 3, 4, 5, 6, 9, 10] and count == 8
    # an explicit anchor (residue 7 alone): the generated residues are still forced; keys are distances to x = 9
    am = np.zeros(12, bool)
    am[7] = True
    index, _, count, _ = select_ref(ca, gen, 4, 0, 4, anchor_mask=am, chain=chain)
    assert index.tolist() == [3, 4, 7, 10] and count == 4  # forced 3, 4, 7, then residue 10 (key 1; residue 6 has key 16)
    # no antigen pass, no chain table (one chain: residue 8 is not flanking anything either), fp32 evaluation gives the same set
    assert select_ref(ca, gen, 5, dtype=np.float32)[0].tolist() == [2, 3, 4, 5, 8]
    # a generated segment whose neighbours are on another chain has no anchor: the generated residues are the anchors
    index, _, count, _ = select_ref(ca, gen, 3, chain=np.array([1, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3, 3]))
    assert index.tolist() == [2, 3, 4] and count == 3  # keys to {3, 4}: residue 2 and residue 5 both 1, the lower index wins
    assert select_ref(ca, np.zeros(12, bool), 4)[2] == 0  # nothing generated
    assert select_ref(ca, gen, 3, chain=chain)[2] == -1  # four forced residues, k = 3


# ------------------------------------------------------------------ C ABI
def header_text():
    return open(os.path.join(REPO, "include", "diffab_hip.h")).read()


def test_header_and_symbol_table_declare_the_three_entries():
    src = header_text()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("diffab_patch_select", "diffab_patch_gather", "diffab_patch_scatter"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _hip.SYMBOLS, name
    assert src.count("preprocess_pdb.py:44-58") >= 3  # each entry cites the reference code it replaces
    limit = int(re.search(r"#define\s+DIFFAB_PATCH_MAX_RESIDUES\s+(\d+)", code).group(1))
    assert limit >= 4096 and limit == patch.MAX_RESIDUES


def test_host_side_refusals_touch_no_gpu():
    """Every refusal below is decided from the scalar arguments and the host row map: the pointers are fake addresses that are never
    dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(0)

    def select(k=8, k_antigen=0, K=8, N=16, antigen=null):
        return l.diffab_patch_select(p, 3, null, p, null, null, antigen, 2, N, k, k_antigen, K, p, p, p, null)

    for kw, word in ((dict(K=7), "cannot hold"), (dict(k=4, k_antigen=5, K=8, antigen=p), "cannot hold"), (dict(k=0), "k must be"),
                     (dict(k_antigen=-1), "k_antigen must be"), (dict(k=4, k_antigen=4), "needs an antigen_mask")):
        rc = select(**kw)
        assert rc == -1 and word in l.diffab_last_error().decode(), (kw, rc, l.diffab_last_error())
    assert select(N=patch.MAX_RESIDUES + 1) == -2 and "at most" in l.diffab_last_error().decode()
    rows = (ctypes.c_int32 * 3)(0, 2, 1)
    assert l.diffab_patch_gather(p, p, rows, 2, 16, 3, 8, 12, p, null) == -1 and "complex_of_row[1] = 2" in l.diffab_last_error().decode()
    rows[1] = -1
    assert l.diffab_patch_gather(p, p, rows, 2, 16, 3, 8, 12, p, null) == -1
    assert l.diffab_patch_gather(p, p, None, 2, 16, 3, 8, 12, p, null) == -1 and "rows must equal B" in l.diffab_last_error().decode()
    assert l.diffab_patch_gather(p, p, None, 2, 16, 2, 8, 0, p, null) == -1 and "row_bytes" in l.diffab_last_error().decode()
    assert l.diffab_patch_scatter(p, p, null, 2, 16, 8, 0, p, null) == -1 and "row_bytes" in l.diffab_last_error().decode()
    assert l.diffab_patch_scatter(p, p, null, -1, 16, 8, 4, p, null) == -1
    assert l.diffab_patch_scatter(null, p, null, 2, 16, 8, 4, p, null) == -1 and "null" in l.diffab_last_error().decode()
    # empty problems return 0 before any pointer is looked at
    assert l.diffab_patch_select(null, 3, null, null, null, null, null, 0, 16, 8, 0, 8, null, null, null, null) == 0
    assert l.diffab_patch_gather(null, null, None, 0, 16, 0, 8, 12, null, null) == 0
    assert l.diffab_patch_scatter(null, null, null, 0, 16, 8, 12, null, null) == 0


# ------------------------------------------------------------------ argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def small_batch(B=2, N=20):
    gm = torch.zeros(B, N, dtype=torch.bool)
    gm[:, 5:8] = True
    return {"seq_idx": torch.zeros(B, N, dtype=torch.long), "xyz": torch.zeros(B, N, 4, 3), "orientations": torch.eye(3).expand(B, N, 3, 3),
            "generation_mask": gm, "chain_idx": torch.ones(B, N, dtype=torch.long), "atom_mask": torch.ones(B, N, 4)}


def small_patch(B=2, K=8):
    return patch.PatchIndex(torch.arange(K).repeat(B, 1), torch.ones(B, K, dtype=torch.bool), torch.full((B,), K, dtype=torch.int32))


def test_select_reaches_the_library_with_good_arguments(no_library):
    b = small_batch()
    with pytest.raises(ReachedTheLibrary):
        patch.select(b["xyz"], b["generation_mask"], k=8)


@pytest.mark.parametrize("kw, match", [
    (dict(k=0), "k must be an int >= 1"), (dict(k=True), "k must be"), (dict(k=8.0), "k must be"), (dict(k_antigen=-1), "k_antigen must be"),
    (dict(k_antigen=4), "needs an antigen_mask"), (dict(pad_to=0), "pad_to must be"),
    (dict(antigen_mask=torch.zeros(2, 20)), "antigen_mask must be a bool tensor"),
    (dict(antigen_mask=torch.zeros(2, 19, dtype=torch.bool)), r"antigen_mask is \(2, 19\)"),
    (dict(anchor_mask=torch.zeros(2, 20, dtype=torch.uint8)), "anchor_mask must be a bool tensor"),
    (dict(residue_mask=torch.zeros(3, 20, dtype=torch.bool)), "residue_mask is"),
    (dict(chain_idx=torch.zeros(2, 20)), "chain_idx must be an integer tensor"),
    (dict(chain_idx=torch.zeros(2, 21, dtype=torch.long)), "chain_idx is"),
])
def test_select_argument_errors(no_library, kw, match):
    b = small_batch()
    with pytest.raises(ValueError, match=match):
        patch.select(b["xyz"], b["generation_mask"], **kw)


def test_select_shape_errors(no_library):
    b = small_batch()
    with pytest.raises(ValueError, match="xyz must be a float tensor"):
        patch.select(torch.zeros(2, 20, 4), b["generation_mask"])
    with pytest.raises(ValueError, match="needs the CA slot"):
        patch.select(torch.zeros(2, 20, 1, 3), b["generation_mask"])
    with pytest.raises(ValueError, match="generation_mask must be a bool tensor"):
        patch.select(b["xyz"], b["generation_mask"].long())
    with pytest.raises(ValueError, match="generation_mask is"):
        patch.select(b["xyz"], b["generation_mask"][:, :10])
    with pytest.raises(ValueError, match="at most 4096"):
        patch.select(torch.zeros(1, 4097, 3), torch.zeros(1, 4097, dtype=torch.bool))


def test_gather_and_paste_argument_errors(no_library):
    b, pi = small_batch(), small_patch()
    with pytest.raises(ReachedTheLibrary):
        patch.gather(b, pi)
    with pytest.raises(ValueError, match="must be the PatchIndex"):
        patch.gather(b, (pi.index, pi.mask))
    with pytest.raises(ValueError, match="malformed PatchIndex"):
        patch.gather(b, patch.PatchIndex(pi.index.int(), pi.mask, pi.count))
    with pytest.raises(ValueError, match="atom_mask is"):
        patch.gather(dict(b, atom_mask=torch.ones(2, 19, 4)), pi)
    with pytest.raises(ValueError, match="no 'seq_idx'"):
        patch.gather({"xyz": b["xyz"]}, pi)
    with pytest.raises(ValueError, match=r"expected \(3, 20"):
        patch.gather(b, small_patch(B=3))
    s = {"seq_idx": torch.zeros(4, 8, dtype=torch.long), "translations": torch.zeros(4, 8, 3), "orientations": torch.zeros(4, 8, 3, 3)}
    with pytest.raises(ReachedTheLibrary):
        patch.paste(b, pi, s, num_samples=2)
    with pytest.raises(ValueError, match="4 design rows for 2 complexes x num_samples = 3"):
        patch.paste(b, pi, s, num_samples=3)
    with pytest.raises(ValueError, match="num_samples must be"):
        patch.paste(b, pi, s, num_samples=0)
    with pytest.raises(ValueError, match="outside"):
        patch.paste(b, pi, s, context_index=torch.tensor([0, 1, 2, 0]))
    with pytest.raises(ValueError, match="one entry per design row"):
        patch.paste(b, pi, s, context_index=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="not both"):
        patch.paste(b, pi, s, num_samples=2, context_index=torch.tensor([0, 0, 1, 1]))
    with pytest.raises(ValueError, match=r"samples\['translations'\] is"):
        patch.paste(b, pi, dict(s, translations=torch.zeros(4, 7, 3)), num_samples=2)
    with pytest.raises(ValueError, match="samples must hold"):
        patch.paste(b, pi, {"seq_idx": s["seq_idx"]}, num_samples=2)
    with pytest.raises(ValueError, match="no 'orientations'"):
        patch.paste({k: v for k, v in b.items() if k != "orientations"}, pi, s, num_samples=2)


def test_design_complex_argument_errors(no_library):
    model = types.SimpleNamespace()  # design_complex bound to a stand-in (a DiffAb builds its IGSO3 tables on the device)
    model.design_complex = types.MethodType(DiffAb.design_complex, model)
    b = small_batch()
    with pytest.raises(ValueError, match="come from the batch"):
        model.design_complex(b, k=8, chain_idx=b["chain_idx"])
    with pytest.raises(ValueError, match="batch must be a dict with xyz and generation_mask"):
        model.design_complex({"xyz": b["xyz"]}, k=8)
    with pytest.raises(ValueError, match="k must be"):
        model.design_complex(b, k=0)
    with pytest.raises(ReachedTheLibrary):
        model.design_complex(b, k=8, pad_to=8)


# ------------------------------------------------------------------ PDB reader
def three_chains(seed=3):
    """A synthetic three-chain backbone (heavy 9, light 7, antigen 11 residues) with a numbering gap inside the heavy chain."""
    g = torch.Generator().manual_seed(seed)
    n = 27
    chain = torch.tensor([1] * 9 + [2] * 7 + [3] * 11)
    ridx = torch.arange(n)
    ridx[5:] += 4  # residues 4 -> 9: a gap inside the heavy chain
    seq = torch.randint(0, 20, (n,), generator=g)
    t = torch.cumsum(torch.randn(n, 3, generator=g) * 2.2, 0)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    O = q * torch.sign(torch.linalg.det(q))[:, None, None]
    return seq, t, O, chain, ridx


def test_read_pdb_round_trips_write_pdb(tmp_path):
    seq, t, O, chain, ridx = three_chains()
    path = str(tmp_path / "c.pdb")
    dio.write_pdb(path, seq, t, O, chain_idx=chain, residue_idx=ridx)
    got = dio.read_pdb(path, heavy="A", light="B", antigen="C")
    assert torch.equal(got["seq_idx"], seq) and torch.equal(got["chain_idx"], chain) and torch.equal(got["residue_idx"], ridx)
    assert torch.equal(got["resseq"], ridx + 1) and bool((got["icode"] == 32).all())
    assert got["antigen_mask"].tolist() == (chain == 3).tolist() and bool(got["residue_mask"].all())
    want = dio.backbone_from_frames(t, O, ("N", "CA", "C", "O"))
    assert got["xyz"].shape == (27, 15, 3) and float((got["xyz"][:, :4] - want).abs().max()) <= 0.0005 + 1e-5  # %8.3f rounding
    assert bool((got["atom_mask"][:, :4] == 1).all()) and bool((got["atom_mask"][:, 4:] == 0).all())
    # all chains, in file order, none of them antigen; a subset and another order by name
    every = dio.read_pdb(path)
    assert torch.equal(every["chain_idx"], chain) and not bool(every["antigen_mask"].any())
    sub = dio.read_pdb(path, heavy="B", antigen=["A"])
    assert sub["chain_idx"].tolist() == [1] * 7 + [3] * 9 and sub["antigen_mask"].tolist() == [False] * 7 + [True] * 9
    assert sub["residue_idx"].tolist() == list(range(7)) + [7, 8, 9, 10, 11, 16, 17, 18, 19]
    with pytest.raises(ValueError, match="no ATOM records of chain 'Z'"):
        dio.read_pdb(path, heavy="Z")


def test_read_pdb_masks_and_ignores(tmp_path):
    """A missing CA masks the residue; altloc B, hydrogens, HETATM and MODEL 2 are ignored; side-chain atoms follow the backbone in the
    record's order; an unknown residue name is UNK; insertion codes start new residues."""
    def atom(serial, name, alt, res, ch, num, icode, x, el, rec="ATOM  "):
        return f"{rec}{serial:5d} {name:<4s}{alt}{res:>3s} {ch}{num:4d}{icode}   {x:8.3f}{x + 1:8.3f}{x + 2:8.3f}{1.0:6.2f}{0.0:6.2f}          {el:>2s}"

    lines = ["MODEL        1",
             atom(1, "N", " ", "SER", "H", 100, " ", 1.0, "N"), atom(2, "CA", "A", "SER", "H", 100, " ", 2.0, "C"),
             atom(3, "CA", "B", "SER", "H", 100, " ", 9.0, "C"), atom(4, "C", " ", "SER", "H", 100, " ", 3.0, "C"),
             atom(5, "OG", " ", "SER", "H", 100, " ", 5.0, "O"), atom(6, "O", " ", "SER", "H", 100, " ", 4.0, "O"),
             atom(7, "CB", " ", "SER", "H", 100, " ", 6.0, "C"), atom(8, "HA", " ", "SER", "H", 100, " ", 7.0, "H"),
             atom(9, "N", " ", "MSE", "H", 100, "A", 11.0, "N"), atom(10, "C", " ", "MSE", "H", 100, "A", 13.0, "C"),
             atom(11, "N", " ", "GLY", "H", 102, " ", 21.0, "N"), atom(12, "CA", " ", "GLY", "H", 102, " ", 22.0, "C"),
             atom(13, "C", " ", "GLY", "H", 102, " ", 23.0, "C"), atom(14, "O", " ", "HOH", "H", 200, " ", 50.0, "O", rec="HETATM"),
             "ENDMDL", "MODEL        2", atom(1, "N", " ", "ALA", "H", 300, " ", 70.0, "N"), "ENDMDL", "END"]
    path = str(tmp_path / "m.pdb")
    open(path, "w").write("\n".join(lines) + "\n")
    got = dio.read_pdb(path, heavy="H")
    assert got["seq_idx"].tolist() == [dio.AA3.index("SER"), 20, dio.AA3.index("GLY")]
    assert got["resseq"].tolist() == [100, 100, 102] and got["icode"].tolist() == [32, ord("A"), 32]
    assert got["residue_idx"].tolist() == [0, 1, 3] and got["residue_mask"].tolist() == [True, False, True]
    assert got["xyz"][0, :6, 0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]  # N, CA (altloc A), C, O, then OG, CB as recorded; no HA
    assert got["atom_mask"][0].tolist() == [1.0] * 6 + [0.0] * 9 and got["atom_mask"][1].tolist() == [1.0, 0.0, 1.0] + [0.0] * 12


def test_chothia_cdr_mask_with_insertion_codes():
    # a heavy chain numbered 93, 94, 95 ... 100, 100A, 100B, 100C, 101, 102, 103 and a light chain 23, 24, 34, 35, 49, 50, 56, 57, 88, 89, 97, 98
    h = [93, 94, 95, 96, 97, 98, 99, 100, 100, 100, 100, 101, 102, 103]
    l = [23, 24, 34, 35, 49, 50, 56, 57, 88, 89, 97, 98]
    chain = torch.tensor([1] * len(h) + [2] * len(l) + [3, 3])
    resseq = torch.tensor(h + l + [96, 30])
    want_h = [False, False] + [True] * 11 + [False]
    want_l = [False, True, True, False, False, True, True, False, False, True, True, False]
    assert dio.chothia_cdr_mask(chain, resseq).tolist() == want_h + want_l + [False, False]
    assert dio.chothia_cdr_mask(chain, resseq, cdrs=("H3",)).tolist() == want_h + [False] * 14
    assert dio.chothia_cdr_mask(chain, resseq, cdrs=("L2",)).tolist() == [False] * 14 + [False] * 5 + [True, True] + [False] * 7
    # the light chain's ranges do not apply to the heavy chain and the other way round
    assert dio.chothia_cdr_mask(torch.tensor([1, 2]), torch.tensor([89, 100])).tolist() == [False, False]
    assert dio.chothia_cdr_mask(torch.tensor([1, 1, 1, 1]), torch.tensor([25, 26, 32, 33]), cdrs=["H1"]).tolist() == [False, True, True, False]
    with pytest.raises(ValueError, match="unknown CDR 'H4'"):
        dio.chothia_cdr_mask(chain, resseq, cdrs=("H4",))
    with pytest.raises(ValueError, match="chain_idx is"):
        dio.chothia_cdr_mask(chain, resseq[:-1])
