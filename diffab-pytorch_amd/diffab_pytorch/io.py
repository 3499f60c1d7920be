"""Input and output side of the path: a PDB reader for whole complexes with the Chothia CDR ranges,
backbone atoms from the sampled frames, a PDB writer and a round-trippable sample file.  The reference stops at frames (x, O) - it has no reconstruction or writer - so this is new,
build-defined functionality (nothing here is on the timed path); the atom reconstruction of frames that live on the device runs on
the HIP frame kernel, file writing is host code.

Frame convention (the one the hot path uses everywhere: reference ``euclidean_transform`` diffab_pytorch.py:315-324,
``global = local @ R + t`` with row vectors): a residue's frame has its origin at CA, and in LOCAL coordinates
C lies on +x and N in the xy-plane with positive y - the Gram-Schmidt frame of AlphaFold-style backbones.
``frames_from_backbone`` and ``backbone_from_frames`` are exact inverses on ideal backbones.  Whether this is the convention
of ``protstruc.StructureBatch.backbone_orientations`` (which produces the reference's orientations, data.py:82) cannot be
checked here (protstruc is not in the tree): parity with it is UNPINNED.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

# ideal local coordinates (Angstrom) of the backbone atoms in the residue frame above (AlphaFold 2 supplementary table 2 geometry)
IDEAL_BACKBONE = {
    "N": (-0.525, 1.363, 0.000),
    "CA": (0.000, 0.000, 0.000),
    "C": (1.526, 0.000, 0.000),
    "O": (2.153, -1.062, 0.000),   # carbonyl oxygen for an extended chain (psi-independent placement in the N-CA-C plane)
    "CB": (-0.529, -0.774, -1.205),
}
BACKBONE_ATOMS = ("N", "CA", "C", "O", "CB")
AA3 = ("ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP",
       "TYR", "VAL", "UNK")  # index order of the 20 + UNK vocabulary (reference AA.UNK = 20)
AA1 = "ARNDCQEGHILKMFPSTWYVX"  # one-letter codes in AA3 order, X = UNK


def _aa_indices(letters: str, V: int, what: str) -> list:
    out = []
    for c in str(letters).upper():
        i = AA1.find(c)
        if i < 0 or i >= V:
            raise ValueError(f"allowed_aa_mask: unknown amino-acid letter {c!r} in {what} (expected letters of {AA1[:V]!r})")
        out.append(i)
    return out


def allowed_aa_mask(K: int, *, exclude: str = "", fixed: Optional[Dict[int, str]] = None, V: int = 21) -> torch.Tensor:
    """(K, V) bool mask for ``DiffAb.sample(allowed_aa=...)`` from one-letter codes (``AA1``: ARNDCQEGHILKMFPSTWYV in AA3 order, X for
    UNK).  Every class is allowed except the letters of ``exclude`` (e.g. "CMX": no Cys, Met or UNK); ``fixed`` maps a residue position
    to a letter or a string of letters, and that position allows exactly those classes (the exclusion list does not apply to it).
    Unknown letters, positions outside [0, K) and an empty set at a fixed position raise ValueError."""
    mask = torch.ones(K, V, dtype=torch.bool)
    mask[:, _aa_indices(exclude, V, "exclude")] = False
    for pos, letters in (fixed or {}).items():
        if isinstance(pos, bool) or not isinstance(pos, int) or not 0 <= pos < K:
            raise ValueError(f"allowed_aa_mask: fixed position {pos!r} outside [0, {K})")
        idx = _aa_indices(letters, V, f"fixed[{pos}]")
        if not idx:
            raise ValueError(f"allowed_aa_mask: fixed[{pos}] allows no class")
        mask[pos] = False
        mask[pos, idx] = True
    return mask


def backbone_from_frames(translations: torch.Tensor, orientations: torch.Tensor, atoms: Sequence[str] = BACKBONE_ATOMS) -> torch.Tensor:
    """(…,3) CA positions and (…,3,3) orientations -> (…, len(atoms), 3) atom coordinates: local @ R + t.
    Frames on the device (the sampler's output) go through the HIP frame kernel - the same `diffab_frames_apply` that implements
    the reference's euclidean_transform (diffab_pytorch.py:315-324), with the ideal backbone as the local points; host tensors
    (files being written) use the identical expression in torch."""
    local = torch.tensor([IDEAL_BACKBONE[a] for a in atoms], dtype=torch.float32)  # (A,3)
    if translations.is_cuda:
        from . import _hip

        lib = _hip.lib()
        t = _hip.dev_f32(translations).reshape(-1, 3)
        R = _hip.dev_f32(orientations).reshape(-1, 3, 3)
        L, A = t.shape[0], len(atoms)
        pts = local.to(t.device).expand(L, A, 3).contiguous()  # (B=1, N=1, L, A, 3)
        out = torch.empty_like(pts)
        _hip.check(lib.diffab_frames_apply(_hip.ptr(pts), _hip.ptr(R), _hip.ptr(t), _hip.ptr(out), 1, 1, L, A, _hip.stream_ptr()),
                   "diffab_frames_apply")
        return out.view(*translations.shape[:-1], A, 3).to(translations.dtype)
    local = local.to(dtype=translations.dtype)
    return torch.einsum("ak,...kc->...ac", local, orientations) + translations.unsqueeze(-2)


def frames_from_backbone(n: torch.Tensor, ca: torch.Tensor, c: torch.Tensor):
    """Inverse of ``backbone_from_frames`` on (N, CA, C): Gram-Schmidt, rows of R are the local axes in global coordinates."""
    e1 = torch.nn.functional.normalize(c - ca, dim=-1)
    u2 = (n - ca) - (e1 * (n - ca)).sum(-1, keepdim=True) * e1
    e2 = torch.nn.functional.normalize(u2, dim=-1)
    e3 = torch.cross(e1, e2, dim=-1)
    return ca, torch.stack([e1, e2, e3], dim=-2)


def _atom_lines(seq_idx, translations, orientations, chain_idx, residue_idx, residue_mask, b_factor, atoms) -> list:
    """ATOM records of one patch (K residues; glycine gets no CB), serial numbers from 1."""
    seq_idx, translations, orientations = seq_idx.cpu(), translations.cpu().float(), orientations.cpu().float()
    K = seq_idx.shape[0]
    xyz = backbone_from_frames(translations, orientations, atoms)
    lines, serial = [], 1
    for i in range(K):
        if residue_mask is not None and not bool(residue_mask[i]):
            continue
        aa = AA3[int(seq_idx[i])] if 0 <= int(seq_idx[i]) < len(AA3) else "UNK"
        ch = "A" if chain_idx is None else chr(ord("A") + max(int(chain_idx[i]) - 1, 0) % 26)
        rn = i + 1 if residue_idx is None else int(residue_idx[i]) + 1
        bf = 0.0 if b_factor is None else float(b_factor[i])
        for a, name in enumerate(atoms):
            if name == "CB" and aa == "GLY":
                continue
            x, y, z = (float(v) for v in xyz[i, a])
            lines.append(f"ATOM  {serial:5d} {name:<4s} {aa:>3s} {ch}{rn:4d}    {x:8.3f}{y:8.3f}{z:8.3f}{1.0:6.2f}{bf:6.2f}          {name[0]:>2s}")
            serial += 1
    return lines


def write_pdb(path: str, seq_idx: torch.Tensor, translations: torch.Tensor, orientations: torch.Tensor,
              chain_idx: Optional[torch.Tensor] = None, residue_idx: Optional[torch.Tensor] = None, residue_mask: Optional[torch.Tensor] = None,
              b_factor: Optional[torch.Tensor] = None, atoms: Sequence[str] = ("N", "CA", "C", "O")) -> int:
    """One patch (K residues) as ATOM records (glycine gets no CB).  chain ids 1, 2, 3 ... -> A, B, C ...; returns the atom count."""
    lines = _atom_lines(seq_idx, translations, orientations, chain_idx, residue_idx, residue_mask, b_factor, atoms)
    n = len(lines)
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return n


# Chothia-scheme CDR ranges by author residue number, ends included (insertion codes belong to their number)
CHOTHIA_CDRS = {"H1": (1, 26, 32), "H2": (1, 52, 56), "H3": (1, 95, 102), "L1": (2, 24, 34), "L2": (2, 50, 56), "L3": (2, 89, 97)}
_BACKBONE_SLOTS = {"N": 0, "CA": 1, "C": 2, "O": 3}


def read_pdb(path: str, *, heavy: Optional[str] = None, light: Optional[str] = None, antigen=None, n_atoms: int = 15) -> Dict[str, torch.Tensor]:
    """A whole complex from a PDB file, as the per-residue fields ``patch.select`` / ``DiffAb.design_complex`` take (no batch axis:
    stack or unsqueeze(0) them).  ATOM records of the first model; of alternate locations the first one met per atom; hydrogens and OXT
    are left out.  ``heavy`` / ``light`` name one chain each, ``antigen`` a chain id or a sequence of them; the residues come in that
    order (heavy, light, antigen chains as listed), ``chain_idx`` 1 heavy, 2 light, 3, 4, ... the antigen chains - write_pdb's A, B, C
    - and ``antigen_mask`` marks the antigen.  With no chain named every chain is read in file order, numbered from 1, none antigen.

    ``seq_idx`` (N,) int64 in ``AA3`` order (unknown residue names -> UNK); ``xyz`` (N, n_atoms, 3) with N, CA, C, O in slots 0-3 and
    the side-chain heavy atoms behind them in the record's order (atoms beyond n_atoms are dropped), ``atom_mask`` (N, n_atoms)
    float32; ``resseq`` (N,) int64 and ``icode`` (N,) uint8 (the character code, 32 = none) as read; ``residue_idx`` (N,) int64: 0
    at the first residue, one more per residue, plus the gap where the author numbering jumps inside a chain (a new chain continues
    one after the last); ``residue_mask`` false where N, CA or C is missing.  The slot order behind the backbone is this project's
    own: parity with protstruc's atom order is UNPINNED.  A named chain that the file does not have raises ValueError."""
    ag = [] if antigen is None else ([antigen] if isinstance(antigen, str) else list(antigen))
    named = [(c, n) for c, n in ((heavy, 1), (light, 2))] + [(c, 3 + j) for j, c in enumerate(ag)]
    named = [(c, n) for c, n in named if c is not None]
    if n_atoms < 4:
        raise ValueError("read_pdb: n_atoms must hold the backbone slots N, CA, C, O (>= 4)")
    chains: Dict[str, list] = {}  # chain id -> residues in file order, each [resname, resseq, icode, {atom name: xyz}, [side-chain names]]
    with open(path) as f:
        for line in f:
            rec = line[:6]
            if rec.startswith("ENDMDL"):
                break
            if rec != "ATOM  " or len(line) < 54:
                continue
            name, element = line[12:16].strip(), line[76:78].strip().upper()
            if element == "H" or element == "D" or (not element and name.lstrip("0123456789")[:1] in ("H", "D")) or name == "OXT":
                continue
            ch = line[21]
            if named and ch not in [c for c, _ in named]:
                continue
            key = (line[17:20].strip().upper(), int(line[22:26]), line[26])
            res = chains.setdefault(ch, [])
            if not res or tuple(res[-1][:3]) != key:
                res.append([*key, {}, []])
            atoms, side = res[-1][3], res[-1][4]
            if name in atoms:  # a later alternate location of an atom already read
                continue
            atoms[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
            if name not in _BACKBONE_SLOTS:
                side.append(name)
    order = named if named else [(c, j + 1) for j, c in enumerate(chains)]
    for c, _ in order:
        if c not in chains:
            raise ValueError(f"read_pdb: {path} has no ATOM records of chain {c!r} (chains: {sorted(chains)})")
    n = sum(len(chains[c]) for c, _ in order)
    out = {"seq_idx": torch.full((n,), len(AA3) - 1, dtype=torch.int64), "xyz": torch.zeros(n, n_atoms, 3),
           "atom_mask": torch.zeros(n, n_atoms), "chain_idx": torch.zeros(n, dtype=torch.int64),
           "residue_idx": torch.zeros(n, dtype=torch.int64), "resseq": torch.zeros(n, dtype=torch.int64),
           "icode": torch.full((n,), 32, dtype=torch.uint8), "antigen_mask": torch.zeros(n, dtype=torch.bool),
           "residue_mask": torch.zeros(n, dtype=torch.bool)}
    i, ridx = 0, -1
    for c, number in order:
        prev = None
        for resname, resseq, icode, atoms, side in chains[c]:
            ridx += 1 if prev is None else max(1, resseq - prev)
            prev = resseq
            out["seq_idx"][i] = AA3.index(resname) if resname in AA3 else len(AA3) - 1
            slots = [(s, a) for a, s in _BACKBONE_SLOTS.items() if a in atoms] + [(4 + j, a) for j, a in enumerate(side) if 4 + j < n_atoms]
            for s, a in slots:
                out["xyz"][i, s] = torch.tensor(atoms[a])
                out["atom_mask"][i, s] = 1.0
            out["chain_idx"][i], out["residue_idx"][i], out["resseq"][i], out["icode"][i] = number, ridx, resseq, ord(icode)
            out["antigen_mask"][i] = bool(named) and number >= 3
            out["residue_mask"][i] = all(a in atoms for a in ("N", "CA", "C"))
            i += 1
    return out


def chothia_cdr_mask(chain_idx: torch.Tensor, resseq: torch.Tensor, cdrs: Sequence[str] = ("H1", "H2", "H3", "L1", "L2", "L3")) -> torch.Tensor:
    """The ``generation_mask`` of a Chothia-numbered structure (such as the reference's data/all_structures/chothia): true where the
    residue's author number lies in one of the named CDRs of its chain - heavy (chain_idx 1) H1 26-32, H2 52-56, H3 95-102; light
    (chain_idx 2) L1 24-34, L2 50-56, L3 89-97, ends included.  An insertion code belongs to its number (100A-100C are in H3), so only
    ``resseq`` is needed.  These are the scheme's published ranges; parity with protstruc.get_cdr_mask is UNPINNED."""
    unknown = [c for c in cdrs if c not in CHOTHIA_CDRS]
    if unknown:
        raise ValueError(f"chothia_cdr_mask: unknown CDR {unknown[0]!r} (expected some of {sorted(CHOTHIA_CDRS)})")
    chain_idx, resseq = torch.as_tensor(chain_idx), torch.as_tensor(resseq)
    if chain_idx.shape != resseq.shape:
        raise ValueError(f"chothia_cdr_mask: chain_idx is {tuple(chain_idx.shape)}, resseq is {tuple(resseq.shape)}")
    mask = torch.zeros(chain_idx.shape, dtype=torch.bool, device=chain_idx.device)
    for c in cdrs:
        chain, lo, hi = CHOTHIA_CDRS[c]
        mask |= (chain_idx == chain) & (resseq >= lo) & (resseq <= hi)
    return mask


def chothia_cdr_index(chain_idx: torch.Tensor, resseq: torch.Tensor) -> torch.Tensor:
    """int64 labels 0..5 for H1, H2, H3, L1, L2, L3 (the ranges of ``chothia_cdr_mask``) and -1 elsewhere: the ``segment_idx`` of
    ``metrics.evaluate`` for per-CDR numbers.  ``chothia_cdr_index(...) >= 0`` equals ``chothia_cdr_mask(...)``."""
    chain_idx, resseq = torch.as_tensor(chain_idx), torch.as_tensor(resseq)
    if chain_idx.shape != resseq.shape:
        raise ValueError(f"chothia_cdr_index: chain_idx is {tuple(chain_idx.shape)}, resseq is {tuple(resseq.shape)}")
    index = torch.full(chain_idx.shape, -1, dtype=torch.int64, device=chain_idx.device)
    for label, c in enumerate(("H1", "H2", "H3", "L1", "L2", "L3")):
        chain, lo, hi = CHOTHIA_CDRS[c]
        index[(chain_idx == chain) & (resseq >= lo) & (resseq <= hi)] = label
    return index


def write_trajectory_pdb(path: str, trajectory: Dict[str, torch.Tensor], row: int, *, predictions: bool = False,
                         chain_idx: Optional[torch.Tensor] = None, residue_idx: Optional[torch.Tensor] = None,
                         residue_mask: Optional[torch.Tensor] = None, atoms: Sequence[str] = ("N", "CA", "C", "O")) -> int:
    """State row ``row`` of ``DiffAb.sample(trajectory=...)['trajectory']`` as a multi-model PDB: one MODEL / ENDMDL per label, in the
    trajectory's label order (descending t; MODEL serial = the label t).  The frames are the recorded state (translations,
    orientations, seq_idx), or with ``predictions=True`` the predicted clean structure (pred_translations, pred_orientations) with the
    argmax of seq_probs as the residue.  The b-factor is the probability of the written residue under seq_probs when the trajectory has
    that field (0 otherwise).  chain_idx / residue_idx / residue_mask are the patch's (K,), as in write_pdb.  Returns the atom count
    of all models."""
    if predictions and "seq_probs" not in trajectory:
        raise ValueError("write_trajectory_pdb: predictions=True needs a trajectory recorded with trajectory_predictions=True")
    labels = trajectory["t"].cpu()
    if predictions:
        probs = trajectory["seq_probs"][row].cpu().float()
        seq = probs.argmax(-1)
        x, O = trajectory["pred_translations"][row], trajectory["pred_orientations"][row]
    else:
        seq, x, O = trajectory["seq_idx"][row].cpu(), trajectory["translations"][row], trajectory["orientations"][row]
        probs = trajectory["seq_probs"][row].cpu().float() if "seq_probs" in trajectory else None
    lines, n = [], 0
    for j in range(labels.numel()):
        bf = None if probs is None else probs[j].gather(-1, seq[j].unsqueeze(-1)).squeeze(-1)
        model = _atom_lines(seq[j], x[j], O[j], chain_idx, residue_idx, residue_mask, bf, atoms)
        n += len(model)
        lines += [f"MODEL     {int(labels[j]):4d}"] + model + ["ENDMDL"]
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return n


def _to_cpu(v):
    if isinstance(v, dict):
        return {k: _to_cpu(u) for k, u in v.items()}
    return v.detach().cpu() if isinstance(v, torch.Tensor) else v


def save_samples(path: str, samples: Dict[str, torch.Tensor], **meta) -> None:
    """``DiffAb.sample`` output (seq_idx, translations, orientations, ...) + free-form metadata, bit-exact round trip.  Nested dicts of
    tensors (sample()'s ``trajectory``, score()'s ``noised``) are saved as nested dicts."""
    torch.save({"samples": _to_cpu(samples), "meta": meta}, path)


def load_samples(path: str):
    d = torch.load(path, map_location="cpu")
    return d["samples"], d.get("meta", {})
