"""Design metrics on the device: what came out of ``DiffAb.sample`` next to the native and next to each other.

``evaluate``        per design: amino-acid recovery, RMSD in the fixed framework and after superposition, whole row and per segment (CDR);
``pairwise``        per patch: the N x N RMSD and sequence-identity matrices of its N designs;
``select_diverse``  greedy farthest-point choice of m designs per patch from such a matrix;
``cluster``         per patch: its designs grouped into families by neighbour count at a distance cutoff of such a matrix - labels, centres,
                    sizes, one representative each; ``cluster_weights`` turns a family into ``ensemble``'s weights (DESIGN section 4.21,
                    ``csrc/cluster_kernels.hip``);
``pareto``          per patch: its designs ranked into non-dominated fronts over several objectives at once, some minimised, some
                    maximised, with hard limits by constrained domination - ranks, front sizes, domination counts, a best-first
                    order and the mask of front 0 (``csrc/pareto_kernels.hip``);
``backbone``      per design: phi, psi, omega and the peptide-bond lengths of the frames' own N, CA, C, chain breaks and cis bonds;
``contacts``        per design: atom clashes of the generated residues against the patch, and their contacts with the antigen;
``contact_map``     per design: the same contacts as data - which generated residue touches which antigen residue, packed as bits;
``pairwise_bits``   per patch: the overlap of such bit sets between all its designs - common contacts, the fraction of common contacts
                    (FCC) and Jaccard, the matrix ``cluster`` turns into binding-mode families (DESIGN section 4.23,
                    ``csrc/interface_kernels.hip``);
``patches``         per design: hydrophobic and charged surface patches of the CDRs and of what they sit on, on one site per residue -
                    the aggregation and polyspecificity side of developability;
``liabilities``     per design: sequence motifs along the chain that do not survive production (N-glycosylation sequons, deamidation,
                    isomerisation and fragmentation sites, free Cys, Met), counted where they touch the design; ``motif_masks`` parses
                    the patterns (``csrc/develop_kernels.hip``);
``interface_energy`` per design: a residue-level, distance-binned pair potential between the designed residues and the antigen, the
                    framework and each other, per residue and per single substitution at a designed position, and against the
                    native the share of improved designs - the DiffAb paper's IMP under that potential; ``PairPotential`` holds a
                    table and its bin edges, ``contact_potential`` builds the placeholder default (DESIGN section 4.25,
                    ``csrc/energy_kernels.hip``);
``novelty``         per design: the nearest sequence of a library of known loops by edit distance - is this loop new, is it unique
                    among its siblings - with ``SequenceSet``, ``sequence_set`` / ``sequence_strings`` for the library and
                    ``design_sequences`` for the designs (``csrc/novelty_kernels.hip``);
``conformation``    per design: the nearest loop of a library of known loops of its length by backbone-dihedral distance - is this
                    shape one a loop is known to take, which canonical class is it in - with ``DihedralSet``, ``dihedral_set`` for
                    the library, ``design_dihedrals`` for the designs and ``dihedral_angle`` to read the number (DESIGN section 4.27,
                    ``csrc/conformation_kernels.hip``);
``surface``         per design: solvent-accessible surface of the generated residues and of the antigen, and the area the two bury on
                    each other - the buried surface area of the interface (``csrc/surface_kernels.hip``);
``hbonds``          per design: Kabsch-Sander backbone hydrogen bonds with the peptide-plane O and the amide H they need, the bonds to
                    antigen and framework, and the secondary structure of every residue (``csrc/hbond_kernels.hip``);
``ensemble``        per patch: its N designs as a distribution - amino-acid frequencies, entropy, consensus, mean structure, RMSF, and
                    how typical each design is of its siblings (``csrc/ensemble_kernels.hip``);
``similarity``      per design, without a superposition: lDDT against the native per residue, per design and per segment, and the
                    recovery of the native residue contacts, Fnat (``csrc/similarity_kernels.hip``).

Model-free: nothing here needs a ``DiffAb``.  Designs come as ``sample()`` returns them - ``seq_idx`` (rows,K), ``translations``
(rows,K,3), ``orientations`` (rows,K,3,3) with ``rows = G * group_size``, row ``g * group_size + r`` = design r of patch g - and the masks
per patch, (G,K).  A residue counts when it is generated and inside ``residue_mask``; a mean over no residue is NaN.  The definitions are
the comments of ``diffab_metrics_vs_native`` / ``_pairwise`` / ``_select_diverse`` / ``_backbone`` / ``_contacts`` / ``_ensemble`` /
``_similarity`` in ``include/diffab_hip.h``, of ``diffab_metrics_surface`` in ``include/diffab_hip_analysis.h`` and of ``diffab_metrics_hbonds`` in
``include/diffab_hip_hbonds.h`` and of ``diffab_metrics_cluster`` and ``diffab_metrics_pareto`` in ``include/diffab_hip_cluster.h``
and of ``diffab_metrics_contact_bits`` and ``diffab_metrics_pairwise_bits`` in ``include/diffab_hip_interface.h``
and of ``diffab_metrics_patches`` and ``diffab_metrics_motifs`` in ``include/diffab_hip_develop.h``
and of ``diffab_metrics_pair_energy`` in ``include/diffab_hip_energy.h``
and of ``diffab_metrics_edit_nearest`` and ``diffab_metrics_pack_sequences`` in ``include/diffab_hip_novelty.h``
and of ``diffab_metrics_dihedral_nearest`` and ``diffab_metrics_pack_dihedrals`` in ``include/diffab_hip_conformation.h``;
every number is computed by the HIP kernels of ``csrc/metrics_kernels.hip``, ``csrc/geometry_kernels.hip`` (the filters, DESIGN
section 4.15), ``csrc/ensemble_kernels.hip``, ``csrc/similarity_kernels.hip``, ``csrc/surface_kernels.hip``, ``csrc/hbond_kernels.hip``,
``csrc/cluster_kernels.hip``, ``csrc/pareto_kernels.hip``, ``csrc/interface_kernels.hip``, ``csrc/develop_kernels.hip``, ``csrc/energy_kernels.hip``, ``csrc/novelty_kernels.hip`` and ``csrc/conformation_kernels.hip``, and there is
no torch fallback (``unpack_contact_map`` is plain torch: it reads bits, it computes nothing; ``motif_masks``, ``sequence_set`` and
``dihedral_set`` parse their input on the host; ``conformation`` takes the cosines and sines of the angles in torch, on the device, in
float64 rounded once, and ``dihedral_angle`` is one torch expression for reading a distance).
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
from typing import Dict, Optional, Sequence

import torch

from . import _hip
from .guidance import residue_tables
from .io import AA1, AA3, BACKBONE_ATOMS, backbone_from_frames

MAX_GROUP = 4096  # DIFFAB_METRICS_MAX_GROUP: designs per patch
MAX_K = 4096  # DIFFAB_METRICS_MAX_K
MAX_SEGMENTS = 8  # DIFFAB_METRICS_MAX_SEGMENTS
MAX_CLASSES = 32  # DIFFAB_METRICS_MAX_CLASSES: amino-acid classes of ensemble
ATOMS = {"ca": None, "backbone": ("N", "CA", "C", "O")}
MAX_CONTEXT_ATOMS = 32  # DIFFAB_METRICS_MAX_CONTEXT_ATOMS: atom slots per context residue
CONTACTS_CHUNK_ATOMS = 1024  # DIFFAB_METRICS_CONTACTS_CHUNK_ATOMS: context atoms the contacts kernel stages in LDS per pass
CONTACTS_CHUNK_RESIDUES = 64  # DIFFAB_METRICS_CONTACTS_CHUNK_RESIDUES: context residues per pass
SIMILARITY_MAX_POINTS = 1024  # DIFFAB_METRICS_SIMILARITY_MAX_POINTS: K * P of one patch, staged on chip
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)  # Angstrom
CONTACT_DISTANCE = {"ca": 8.0, "backbone": 5.0}  # similarity's default per atom set
PEPTIDE_BOND = 1.329  # Angstrom, C(i) - N(i+1)
GLY = AA3.index("GLY")
PRO = AA3.index("PRO")  # hbonds(): no amide hydrogen
HBONDS_MAX_K = 512  # DIFFAB_HBONDS_MAX_K: hbonds keeps the K x K bond bits of a row on chip
SS_LETTERS = " HBEGITS"  # hbonds()['ss']: none, alpha helix, lone bridge, ladder, 3-10 helix, pi helix, turn, bend
CLUSTER_LDS_MAX_N = 1024  # DIFFAB_METRICS_CLUSTER_LDS_MAX_N: up to here cluster keeps the N x N neighbour bits of a patch on chip
PARETO_MAX_OBJECTIVES = 16  # DIFFAB_METRICS_PARETO_MAX_OBJECTIVES: objectives of pareto
INTERFACE_MAX_K = 512  # DIFFAB_INTERFACE_MAX_K: residues per patch of a contact map
INTERFACE_MAX_WORDS = 8192  # DIFFAB_INTERFACE_MAX_WORDS: 32-bit words per design of pairwise_bits (a contact map at K = 512)
DEVELOP_MAX_K = 512  # DIFFAB_DEVELOP_MAX_K: residues per patch of patches and liabilities
DEVELOP_MAX_CLASSES = 32  # DIFFAB_DEVELOP_MAX_CLASSES: entries of the two weight tables of patches, classes of a motif word
DEVELOP_MAX_MOTIFS = 32  # DIFFAB_DEVELOP_MAX_MOTIFS: motifs of one liabilities call, one bit of motif_start each
DEVELOP_MOTIF_WORDS = 4  # DIFFAB_DEVELOP_MOTIF_WORDS: a motif is at most four residues long
ENERGY_MAX_K = 512  # DIFFAB_ENERGY_MAX_K: residues per patch of interface_energy
ENERGY_MAX_CLASSES = 32  # DIFFAB_ENERGY_MAX_CLASSES: token classes of a pair potential
ENERGY_MAX_BINS = 8  # DIFFAB_ENERGY_MAX_BINS: distance bins of a pair potential
NOVELTY_MAX_QUERY = 64  # DIFFAB_NOVELTY_MAX_QUERY: tokens of a query of novelty, one bit of a 64-bit word each
NOVELTY_MAX_LIBRARY = 256  # DIFFAB_NOVELTY_MAX_LIBRARY: tokens of a library sequence of novelty, and of any SequenceSet
NOVELTY_CHUNK = 2048  # DIFFAB_NOVELTY_CHUNK: library entries per partial result in novelty's workspace
NOVELTY_PAD = 255  # what stands behind a sequence's last token
CONFORMATION_MAX_LENGTH = 64  # DIFFAB_CONFORMATION_MAX_LENGTH: residues of a loop of conformation, one bit of a 64-bit word each
CONFORMATION_CHUNK = 2048  # DIFFAB_CONFORMATION_CHUNK: sorted library places per partial result in conformation's workspace
DIHEDRALS = ("phi", "psi", "omega")  # the angle kinds of a DihedralSet, in the order of its last axis
SURFACE_MIN_POINTS, SURFACE_MAX_POINTS = 8, 256# DIFFAB_METRICS_SURFACE_MIN_POINTS / _MAX_POINTS: sphere points per atom
# surface(): united-atom radii of the frame atoms in Angstrom (hydrogens folded into the heavy atom) - this project's own choice
ATOM_RADIUS = {"N": 1.65, "CA": 1.87, "C": 1.76, "O": 1.40, "CB": 1.87}


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_dist(who: str, dist) -> tuple:
    """dist (G,N,N) float32 -> (G, N)."""
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.float32 or dist.dim() != 3 or dist.shape[1] != dist.shape[2]:
        raise ValueError(f"{who}: dist must be a float32 tensor (G, N, N)")
    G, N = int(dist.shape[0]), int(dist.shape[1])
    if N < 1 or N > MAX_GROUP:
        raise ValueError(f"{who}: dist has N = {N} designs per patch, outside [1, {MAX_GROUP}]")
    return G, N


def _check_per_design(who: str, G: int, N: int, **tensors) -> None:
    """Optional (G,N) operands, checked in the order given: ``candidates`` is a bool tensor, every other one a float tensor."""
    for name, t in tensors.items():
        kind = "bool" if name == "candidates" else "float"
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (G, N)
                              or not (t.dtype == torch.bool if kind == "bool" else t.is_floating_point())):
            raise ValueError(f"{who}: {name} must be a {kind} tensor {(G, N)}")


def _check_frames(who: str, name: str, d, atoms: str):
    """seq_idx (R,K) integer, translations (R,K,3) float, orientations (R,K,3,3) float (needed for the backbone only) -> (R, K)."""
    if not isinstance(d, dict) or not isinstance(d.get("seq_idx"), torch.Tensor) or not isinstance(d.get("translations"), torch.Tensor):
        raise ValueError(f"{who}: {name} must be a dict with seq_idx and translations (and orientations for atoms='backbone')")
    seq, x = d["seq_idx"], d["translations"]
    if seq.dim() != 2 or seq.is_floating_point() or seq.dtype == torch.bool:
        raise ValueError(f"{who}: {name}['seq_idx'] must be an integer tensor (rows, K), got {tuple(seq.shape)} {seq.dtype}")
    R, K = int(seq.shape[0]), int(seq.shape[1])
    if not x.is_floating_point() or tuple(x.shape) != (R, K, 3):
        raise ValueError(f"{who}: {name}['translations'] is {tuple(x.shape)} {x.dtype}, expected a float tensor {(R, K, 3)}")
    if atoms == "backbone":
        O = d.get("orientations")
        if not isinstance(O, torch.Tensor) or not O.is_floating_point() or tuple(O.shape) != (R, K, 3, 3):
            raise ValueError(f"{who}: {name}['orientations'] must be a float tensor {(R, K, 3, 3)} for atoms='backbone'")
    return R, K


def _check_common(who: str, designs, generation_mask, residue_mask, group_size, atoms):
    if atoms not in ATOMS:
        raise ValueError(f"{who}: atoms must be 'ca' or 'backbone', got {atoms!r}")
    rows, K = _check_frames(who, "designs", designs, atoms)
    if not _is_int(group_size) or group_size < 1:
        raise ValueError(f"{who}: group_size must be an int >= 1, got {group_size!r}")
    if group_size > MAX_GROUP:
        raise ValueError(f"{who}: group_size = {group_size}, at most {MAX_GROUP} designs per patch")
    if rows % group_size != 0:
        raise ValueError(f"{who}: {rows} design rows are not a multiple of group_size = {group_size}")
    if K < 1 or K > MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch outside [1, {MAX_K}]")
    G = rows // group_size
    for name, m in (("generation_mask", generation_mask), ("residue_mask", residue_mask)):
        if m is None and name == "residue_mask":
            continue
        if not isinstance(m, torch.Tensor) or m.dtype != torch.bool:
            raise ValueError(f"{who}: {name} must be a bool tensor")
        if tuple(m.shape) != (G, K):
            raise ValueError(f"{who}: {name} is {tuple(m.shape)}, expected {(G, K)} (one row per patch)")
    return rows, G, K


def _points(d, atoms: str) -> torch.Tensor:
    """(R,K,P,3) fp32 on the device: the CA, or N, CA, C, O from the frames through the frame kernel."""
    x = _hip.dev_f32(d["translations"])
    if atoms == "ca":
        return x.unsqueeze(2).contiguous()
    return _hip.dev_f32(backbone_from_frames(x, _hip.dev_f32(d["orientations"]), ATOMS[atoms]))


def evaluate(designs: Dict[str, torch.Tensor], native: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *,
             residue_mask: Optional[torch.Tensor] = None, segment_idx: Optional[torch.Tensor] = None, num_segments: Optional[int] = None,
             group_size: int = 1, atoms: str = "ca") -> Dict[str, torch.Tensor]:
    """Each design against the native of its patch, over the counted residues: ``aar`` (fraction of native tokens recovered), ``rmsd``
    (no superposition: the framework is fixed, the patch frame is the alignment - the DiffAb number) and ``rmsd_aligned`` (the Kabsch
    minimum over proper rotations and translations), each (rows,).  ``designs`` is the dict ``sample()`` returns (with
    ``design_complex``, its ``out``), ``native`` holds the patch's own ``seq_idx`` (G,K), ``translations`` and ``orientations`` - the
    fields ``sample()`` was called with - and ``group_size`` is its ``num_samples``.  ``atoms``: ``'ca'`` or ``'backbone'`` (N, CA, C,
    O from the frames).  ``segment_idx`` (G,K) integer labels in [0, ``num_segments``) (negative: no segment; ``num_segments`` defaults
    to the largest label + 1, at most 8) adds ``segment_aar``, ``segment_rmsd`` and ``segment_rmsd_aligned`` (rows, num_segments):
    ``io.chothia_cdr_index`` gives the labels of the six CDRs.  One C-ABI call; results on the device of ``designs['seq_idx']``.

    ValueError, naming the argument, before any device work for shapes and dtypes that do not match, rows that are no multiple of
    ``group_size``, more than 8 segments, more than 4096 designs per patch and an unknown ``atoms``."""
    who = "metrics.evaluate()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, atoms)
    nG, nK = _check_frames(who, "native", native, atoms)
    if (nG, nK) != (G, K):
        raise ValueError(f"{who}: native['seq_idx'] is {(nG, nK)}, expected {(G, K)} (one row per patch)")
    S = 0
    if segment_idx is not None:
        if not isinstance(segment_idx, torch.Tensor) or segment_idx.is_floating_point() or segment_idx.dtype == torch.bool:
            raise ValueError(f"{who}: segment_idx must be an integer tensor")
        if tuple(segment_idx.shape) != (G, K):
            raise ValueError(f"{who}: segment_idx is {tuple(segment_idx.shape)}, expected {(G, K)}")
        if num_segments is None:
            num_segments = max(1, int(segment_idx.max()) + 1) if segment_idx.numel() else 1
        if not _is_int(num_segments) or num_segments < 1 or num_segments > MAX_SEGMENTS:
            raise ValueError(f"{who}: num_segments = {num_segments!r} (segment_idx labels up to it) outside [1, {MAX_SEGMENTS}]")
        S = num_segments
    elif num_segments is not None:
        raise ValueError(f"{who}: num_segments without segment_idx")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    P = 1 if atoms == "ca" else len(ATOMS[atoms])
    seq, pts = _hip.dev_i64(designs["seq_idx"]), _points(designs, atoms)
    nseq, npts = _hip.dev_i64(native["seq_idx"]), _points(native, atoms)
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    seg = None if segment_idx is None else _hip.dev_i64(segment_idx)
    whole = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(3)]
    parts = [torch.empty(rows, S, dtype=torch.float32, device=dev) if S else None for _ in range(3)]
    _hip.check(lib.diffab_metrics_vs_native(_hip.ptr(seq), _hip.ptr(pts), _hip.ptr(nseq), _hip.ptr(npts), _hip.ptr(gm), _hip.ptr(rm),
                                            _hip.ptr(seg), rows, group_size, K, P, S, *[_hip.ptr(t) for t in whole + parts],
                                            _hip.stream_ptr()), "diffab_metrics_vs_native")
    out = dict(zip(("aar", "rmsd", "rmsd_aligned"), whole))
    if S:
        out.update(zip(("segment_aar", "segment_rmsd", "segment_rmsd_aligned"), parts))
    return {k: v.to(out_dev) for k, v in out.items()}


def pairwise_workspace_bytes(G: int, N: int, K: int, P: int) -> int:
    """DIFFAB_METRICS_PAIRWISE_WORKSPACE_BYTES of include/diffab_hip.h."""
    return G * N * (K * P * 12 + (K + 3) // 4 * 4 + 32) + G * 4 + 1024


def pairwise(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, residue_mask: Optional[torch.Tensor] = None,
             group_size: int, atoms: str = "ca", aligned: bool = False) -> Dict[str, torch.Tensor]:
    """The designs of each patch against each other, over the patch's counted residues: ``rmsd`` (G,N,N) fp32 - in place, or the Kabsch
    minimum with ``aligned=True`` - and ``seq_identity`` (G,N,N) fp32, the fraction of counted residues with equal tokens;
    N = ``group_size``.  Both are symmetric to the bit; the diagonal is 0 / 1 by definition (NaN for a patch without a counted
    residue).  ``1 - seq_identity`` or ``rmsd`` is a distance matrix for ``select_diverse``.  One C-ABI call (two launches); the
    call's workspace is about the size of the designs' points.  ValueError before any device work as for ``evaluate``."""
    who = "metrics.pairwise()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, atoms)
    if not isinstance(aligned, bool):
        raise ValueError(f"{who}: aligned must be a bool, got {aligned!r}")
    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    N, P = group_size, 1 if atoms == "ca" else len(ATOMS[atoms])
    seq, pts = _hip.dev_i64(designs["seq_idx"]), _points(designs, atoms)
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    rmsd = torch.empty(G, N, N, dtype=torch.float32, device=dev)
    ident = torch.empty(G, N, N, dtype=torch.float32, device=dev)
    nbytes = pairwise_workspace_bytes(G, N, K, P)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_pairwise(_hip.ptr(seq), _hip.ptr(pts), _hip.ptr(gm), _hip.ptr(rm), G, N, K, P, int(aligned), _hip.ptr(rmsd),
                                           _hip.ptr(ident), _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_pairwise")
    return {"rmsd": rmsd.to(out_dev), "seq_identity": ident.to(out_dev)}


def select_diverse(dist: torch.Tensor, m: int, *, score: Optional[torch.Tensor] = None,
                   candidates: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Greedy farthest-point choice of ``m`` designs per patch from ``dist`` (G,N,N) fp32 (``pairwise``'s ``rmsd``, or
    ``1 - seq_identity``).  The first pick is the candidate with the lowest ``score`` (G,N) (ties to the lower index; a NaN score counts
    as +inf), or the first candidate without ``score``; every next pick is the candidate whose smallest distance to the picked ones is
    largest (ties to the lower index, a NaN distance counts as 0).  ``candidates`` (G,N) bool restricts the choice.  Returns ``index``
    (G,m) int64, ``min_dist`` (G,m) fp32 - that smallest distance when the design was picked, +inf for the first - and ``count`` (G,)
    int32; with fewer than ``m`` candidates the tail is -1 / NaN.  Comparisons only: the result is a function of the fp32 matrix."""
    who = "metrics.select_diverse()"
    G, N = _check_dist(who, dist)
    if not _is_int(m) or m < 0:
        raise ValueError(f"{who}: m must be an int >= 0, got {m!r}")
    _check_per_design(who, G, N, score=score, candidates=candidates)
    lib = _hip.lib()
    dev, out_dev = _hip.device(), dist.device
    d = _hip.dev_f32(dist)
    sc = None if score is None else _hip.dev_f32(score)
    cand = None if candidates is None else _hip.dev_mask(candidates)
    index = torch.empty(G, m, dtype=torch.int64, device=dev)
    min_dist = torch.empty(G, m, dtype=torch.float32, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    _hip.check(lib.diffab_metrics_select_diverse(_hip.ptr(d), _hip.ptr(sc), _hip.ptr(cand), G, N, m, _hip.ptr(index), _hip.ptr(min_dist),
                                                 _hip.ptr(count), _hip.stream_ptr()), "diffab_metrics_select_diverse")
    return {"index": index.to(out_dev), "min_dist": min_dist.to(out_dev), "count": count.to(out_dev)}


# ------------------------------------------------------------------ design clusters
def cluster_workspace_bytes(G: int, N: int) -> int:
    """DIFFAB_METRICS_CLUSTER_WORKSPACE_BYTES of include/diffab_hip_cluster.h."""
    Np = (N + 63) // 64 * 64
    return G * (Np * Np // 8 + (N + 255) // 256 * Np * 4) + 1024


def cluster(dist: torch.Tensor, cutoff, *, candidates: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
            max_clusters: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The designs of each patch grouped into families: Daura / GROMOS neighbour-count clustering of ``dist`` (G,N,N) fp32
    (``pairwise``'s ``rmsd``, or ``1 - seq_identity``) at ``cutoff``, a number or a (G,) tensor.  j is a neighbour of i when
    ``dist[g,i,j] <= cutoff[g]`` (the row of i; a NaN is no neighbour; every design is its own).  The open set starts as
    ``candidates`` (G,N) bool (all without it); while it is not empty and fewer than ``max_clusters`` (an int in [0, N]; None = N)
    clusters are made, the open design with the most open neighbours - ties to the lower ``score`` (G,N) (a NaN counts as +inf), then
    to the lower index - becomes a centre, and it and its open neighbours leave as one cluster.

    Returns ``label`` (G,N) int32, the cluster of every design (-1: not a candidate, or still open when ``max_clusters`` was
    reached), ``center_dist`` (G,N) fp32, its distance from its centre as stored in the centre's row (0 for the centre, NaN where the
    label is -1), ``center`` (G,M) int64 and ``size`` (G,M) int32 per cluster, largest first (-1 / 0 past ``count``), ``count`` (G,)
    int32, ``n_unassigned`` (G,) int32, the candidates still open, and ``representative`` (G,N) bool, true at the centres - ready as
    ``select_diverse(candidates=...)`` or as a filter; ``cluster_weights`` makes ``ensemble``'s weights of one cluster.  Compares,
    popcounts and integer adds only: the result is a function of the fp32 matrix.  One C-ABI call (two launches); results on
    ``dist``'s device; ValueError naming the argument before any device work."""
    who = "metrics.cluster()"
    G, N = _check_dist(who, dist)
    if isinstance(cutoff, torch.Tensor):
        if not cutoff.is_floating_point() or tuple(cutoff.shape) != (G,):
            raise ValueError(f"{who}: cutoff must be a number or a float tensor {(G,)}")
    elif isinstance(cutoff, bool) or not isinstance(cutoff, (int, float)):
        raise ValueError(f"{who}: cutoff must be a number or a float tensor {(G,)}, got {cutoff!r}")
    _check_per_design(who, G, N, candidates=candidates, score=score)
    M = N if max_clusters is None else max_clusters
    if not _is_int(M) or M < 0 or M > N:
        raise ValueError(f"{who}: max_clusters must be an int in [0, N = {N}] or None, got {max_clusters!r}")
    lib = _hip.lib()
    dev, out_dev = _hip.device(), dist.device
    d = _hip.dev_f32(dist)
    cut = _hip.dev_f32(cutoff) if isinstance(cutoff, torch.Tensor) else torch.full((G,), float(cutoff), dtype=torch.float32, device=dev)
    sc = None if score is None else _hip.dev_f32(score)
    cand = None if candidates is None else _hip.dev_mask(candidates)
    label = torch.empty(G, N, dtype=torch.int32, device=dev)
    center_dist = torch.empty(G, N, dtype=torch.float32, device=dev)
    center = torch.empty(G, M, dtype=torch.int64, device=dev)
    size = torch.empty(G, M, dtype=torch.int32, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    left = torch.empty(G, dtype=torch.int32, device=dev)
    nbytes = cluster_workspace_bytes(G, N)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_cluster(_hip.ptr(d), _hip.ptr(cut), _hip.ptr(sc), _hip.ptr(cand), G, N, M, _hip.ptr(label),
                                          _hip.ptr(center_dist), _hip.ptr(center), _hip.ptr(size), _hip.ptr(count), _hip.ptr(left),
                                          _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_cluster")
    rep = torch.zeros(G, N + 1, dtype=torch.bool, device=dev)  # (column N takes the -1 padding of center)
    rep.scatter_(1, torch.where(center < 0, N, center), True)
    out = {"label": label, "center_dist": center_dist, "center": center, "size": size, "count": count, "n_unassigned": left,
           "representative": rep[:, :N].contiguous()}
    return {k: v.to(out_dev) for k, v in out.items()}


def cluster_weights(clusters: Dict[str, torch.Tensor], cluster=0) -> torch.Tensor:
    """(G,N) fp32 weights, 1 on the designs of one cluster of ``cluster()``'s result and 0 elsewhere: the mask ``ensemble(weights=...)``
    takes.  ``cluster`` is one index >= 0 for every patch (0: the largest family) or a (G,) integer tensor of indices; an index past a
    patch's ``count`` gives that patch all zeros."""
    who = "metrics.cluster_weights()"
    label = clusters.get("label") if isinstance(clusters, dict) else None
    if not isinstance(label, torch.Tensor) or label.dim() != 2 or label.is_floating_point() or label.dtype == torch.bool:
        raise ValueError(f"{who}: clusters must be the dict metrics.cluster() returns, with an integer label (G, N)")
    G = int(label.shape[0])
    if isinstance(cluster, torch.Tensor):
        if cluster.is_floating_point() or cluster.dtype == torch.bool or tuple(cluster.shape) != (G,):
            raise ValueError(f"{who}: cluster must be an int >= 0 or an integer tensor {(G,)}")
        if G and int(cluster.min()) < 0:
            raise ValueError(f"{who}: cluster holds a negative index (label -1 marks the designs of no cluster)")
        which = cluster.to(device=label.device, dtype=label.dtype)[:, None]
    elif not _is_int(cluster) or cluster < 0:
        raise ValueError(f"{who}: cluster must be an int >= 0 or an integer tensor {(G,)}, got {cluster!r}")
    else:
        which = cluster
    return label.eq(which).to(torch.float32)


# ------------------------------------------------------------------ Pareto fronts
def pareto_workspace_bytes(G: int, N: int) -> int:
    """DIFFAB_METRICS_PARETO_WORKSPACE_BYTES of include/diffab_hip_cluster.h."""
    Np = (N + 63) // 64 * 64
    return G * (Np * Np // 8 + (N + 255) // 256 * Np * 4 + Np // 64 * Np * 4) + 1024


def _objective_table(who: str, objectives, group_size) -> torch.Tensor:
    """(G,N,M) from a (G,N,M) float32 tensor, or from a sequence of M per-design tensors of G * N elements each."""
    if isinstance(objectives, torch.Tensor):
        if objectives.dtype != torch.float32 or objectives.dim() != 3:
            raise ValueError(f"{who}: objectives must be a float32 tensor (G, N, M) or a sequence of per-design tensors, got a "
                             f"{tuple(objectives.shape)} {objectives.dtype} tensor")
        if group_size is not None and (not _is_int(group_size) or group_size != objectives.shape[1]):
            raise ValueError(f"{who}: group_size = {group_size!r} does not match objectives {tuple(objectives.shape)}")
        return objectives
    if not isinstance(objectives, (list, tuple)) or len(objectives) == 0 or not all(isinstance(o, torch.Tensor) for o in objectives):
        raise ValueError(f"{who}: objectives must be a float32 tensor (G, N, M) or a non-empty sequence of per-design tensors")
    if len(objectives) > PARETO_MAX_OBJECTIVES:
        raise ValueError(f"{who}: objectives holds M = {len(objectives)} objectives, outside [1, {PARETO_MAX_OBJECTIVES}]")
    first = objectives[0]
    for m, o in enumerate(objectives):
        if o.dtype == torch.bool or o.is_complex() or o.dim() not in (1, 2):
            raise ValueError(f"{who}: objectives[{m}] must be a float or integer tensor (G * N,) or (G, N), got {tuple(o.shape)} {o.dtype}")
        if tuple(o.shape) != tuple(first.shape):
            raise ValueError(f"{who}: objectives[{m}] is {tuple(o.shape)}, objectives[0] is {tuple(first.shape)}")
    if first.dim() == 2:
        if group_size is not None and (not _is_int(group_size) or group_size != first.shape[1]):
            raise ValueError(f"{who}: group_size = {group_size!r} does not match objectives[0] {tuple(first.shape)}")
        G, N = int(first.shape[0]), int(first.shape[1])
    else:
        if not _is_int(group_size) or group_size < 1:
            raise ValueError(f"{who}: group_size must be an int >= 1 for flat per-design objectives, got {group_size!r}")
        if first.shape[0] % group_size != 0:
            raise ValueError(f"{who}: {first.shape[0]} design rows are not a multiple of group_size = {group_size}")
        G, N = int(first.shape[0]) // group_size, group_size
    return torch.stack([o.to(device=first.device, dtype=torch.float32).reshape(G, N) for o in objectives], dim=-1)


def pareto(objectives, *, group_size: Optional[int] = None, maximize=None, violation: Optional[torch.Tensor] = None,
           score: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None,
           max_fronts: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The designs of each patch ranked into non-dominated fronts over M objectives: Pareto ranking with Deb's constrained domination.
    ``objectives`` is a float32 (G,N,M) tensor, or a sequence of M per-design tensors of G * N elements each, shaped (G * N,) as the
    filters return them (then ``group_size`` = N is required) or (G,N); integer tensors are converted.  Every objective is minimised
    unless ``maximize``, a bool or a sequence of M bools, says otherwise; a NaN is the worst value of its objective.  ``violation``
    (G,N) float is a hard limit's overshoot: values <= 0 are feasible, a smaller violation dominates whatever the objectives say, and a
    NaN is the largest.  i dominates j when both are ``candidates`` (G,N) bool (all without it) and i violates less, or they violate
    alike and i is no worse in every objective and better in one; equal designs share a front.  Front 0 is every candidate nobody
    dominates, front 1 the same among the rest, and so on up to ``max_fronts`` (an int in [0, N]; None = N).

    Returns ``rank`` (G,N) int32 (-1: not a candidate, or still open after ``max_fronts``), ``n_dominators`` and ``n_dominated`` (G,N)
    int32 over all candidates (-1 for a non-candidate), ``front_size`` (G,F) int32 (0 past ``count``), ``count`` (G,) int32,
    ``n_unranked`` (G,) int32, ``order`` (G,N) int64 - a permutation, best first, by (front, ``score`` (G,N) with NaN = +inf, more
    designs dominated first, index), unranked candidates and then non-candidates last, so front r is a slice of it - and ``front``
    (G,N) bool, true where ``rank == 0``: ready for ``select_diverse(candidates=...)`` and, as ``front.float()``, for
    ``ensemble(weights=...)``.  Compares, popcounts and integer adds only: the result is a function of the fp32 inputs.  One C-ABI
    call (two launches); results on the objectives' device; ValueError naming the argument before any device work."""
    who = "metrics.pareto()"
    obj = _objective_table(who, objectives, group_size)
    G, N, M = (int(v) for v in obj.shape)
    if N < 1 or N > MAX_GROUP:
        raise ValueError(f"{who}: objectives has N = {N} designs per patch, outside [1, {MAX_GROUP}]")
    if M < 1 or M > PARETO_MAX_OBJECTIVES:
        raise ValueError(f"{who}: objectives holds M = {M} objectives, outside [1, {PARETO_MAX_OBJECTIVES}]")
    if maximize is None or isinstance(maximize, bool):
        flags = [bool(maximize)] * M
    elif isinstance(maximize, (list, tuple)) and len(maximize) == M and all(isinstance(b, bool) for b in maximize):
        flags = list(maximize)
    else:
        raise ValueError(f"{who}: maximize must be a bool or a sequence of M = {M} bools, got {maximize!r}")
    _check_per_design(who, G, N, violation=violation, score=score, candidates=candidates)
    F = N if max_fronts is None else max_fronts
    if not _is_int(F) or F < 0 or F > N:
        raise ValueError(f"{who}: max_fronts must be an int in [0, N = {N}] or None, got {max_fronts!r}")
    lib = _hip.lib()
    dev, out_dev = _hip.device(), obj.device
    o = _hip.dev_f32(obj)
    mx = torch.tensor(flags, dtype=torch.bool, device=dev) if any(flags) else None
    vio = None if violation is None else _hip.dev_f32(violation)
    sc = None if score is None else _hip.dev_f32(score)
    cand = None if candidates is None else _hip.dev_mask(candidates)
    i32 = dict(dtype=torch.int32, device=dev)
    rank, by, of = (torch.empty(G, N, **i32) for _ in range(3))
    front_size, count, left = torch.empty(G, F, **i32), torch.empty(G, **i32), torch.empty(G, **i32)
    order = torch.empty(G, N, dtype=torch.int64, device=dev)
    nbytes = pareto_workspace_bytes(G, N)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_pareto(_hip.ptr(o), _hip.ptr(mx), _hip.ptr(vio), _hip.ptr(sc), _hip.ptr(cand), G, N, M, F, _hip.ptr(rank),
                                         _hip.ptr(by), _hip.ptr(of), _hip.ptr(front_size), _hip.ptr(count), _hip.ptr(left), _hip.ptr(order),
                                         _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_pareto")
    out = {"rank": rank, "n_dominators": by, "n_dominated": of, "front_size": front_size, "count": count, "n_unranked": left,
           "order": order, "front": rank.eq(0)}
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ design filters
def _check_distance(who: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}")
    return float(v)


def _check_patch_mask(who: str, name: str, m, G: int, K: int) -> None:
    if not isinstance(m, torch.Tensor) or m.dtype != torch.bool:
        raise ValueError(f"{who}: {name} must be a bool tensor")
    if tuple(m.shape) != (G, K):
        raise ValueError(f"{who}: {name} is {tuple(m.shape)}, expected {(G, K)} (one row per patch)")


def _check_atoms(who: str, atoms) -> tuple:
    if isinstance(atoms, str) or not isinstance(atoms, Sequence) or not 1 <= len(atoms) <= len(BACKBONE_ATOMS) \
            or any(a not in BACKBONE_ATOMS for a in atoms) or len(set(atoms)) != len(atoms):
        raise ValueError(f"{who}: atoms must be a sequence of distinct names from {BACKBONE_ATOMS}, got {atoms!r}")
    return tuple(atoms)


def _check_context(who: str, context, G: int, K: int) -> int:
    """A patch's real atoms, xyz (G,K,A,3) and atom_mask (G,K,A) -> A."""
    if not isinstance(context, dict) or not isinstance(context.get("xyz"), torch.Tensor) or not isinstance(context.get("atom_mask"), torch.Tensor):
        raise ValueError(f"{who}: context must be a dict with xyz (G,K,A,3) and atom_mask (G,K,A)")
    xyz, am = context["xyz"], context["atom_mask"]
    if not xyz.is_floating_point() or xyz.dim() != 4 or tuple(xyz.shape[:2]) != (G, K) or xyz.shape[3] != 3:
        raise ValueError(f"{who}: context['xyz'] is {tuple(xyz.shape)} {xyz.dtype}, expected a float tensor {(G, K, 'A', 3)}")
    A = int(xyz.shape[2])
    if A < 1 or A > MAX_CONTEXT_ATOMS:
        raise ValueError(f"{who}: context['xyz'] has A = {A} atoms per residue, outside [1, {MAX_CONTEXT_ATOMS}]")
    if am.is_complex() or tuple(am.shape) != (G, K, A):  # (bool, or the reference batch's 0 / 1 numbers)
        raise ValueError(f"{who}: context['atom_mask'] is {tuple(am.shape)} {am.dtype}, expected a mask {(G, K, A)}")
    return A


def _valid_word(atom_mask: torch.Tensor, A: int, dev) -> torch.Tensor:
    """atom_mask (G,K,A) -> (G,K) int32 holding the A bits of a uint32."""
    word = (_hip.dev_mask(atom_mask).to(torch.int64) << torch.arange(A, device=dev)).sum(-1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).contiguous()


def backbone_workspace_bytes(G: int, K: int) -> int:
    """DIFFAB_METRICS_BACKBONE_WORKSPACE_BYTES of include/diffab_hip.h."""
    return G * K * 8 + 1024


def contacts_workspace_bytes(G: int, K: int, A: int) -> int:
    """DIFFAB_METRICS_CONTACTS_WORKSPACE_BYTES of include/diffab_hip.h."""
    return G * K * (A * 16 + 28) + G * 16 + 2048


def backbone(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, chain_idx=None, residue_idx=None,
             residue_mask: Optional[torch.Tensor] = None, group_size: int = 1, bond_tolerance: float = 0.25) -> Dict[str, torch.Tensor]:
    """The backbone the frames of each design imply - N, CA, C of ``io.backbone_from_frames``, the atoms ``write_pdb`` writes - checked
    where residues join.  Slots i and j are chain neighbours when ``chain_idx`` is equal, ``residue_idx[j] = residue_idx[i] + 1`` and both
    are inside ``residue_mask`` (the bonded rule of guidance; ``chain_idx`` / ``residue_idx`` are (K,) or (G,K), default one chain and
    ``arange(K)``).  Per residue (rows,K) fp32, NaN where the neighbour it needs does not exist: ``phi``, ``psi``, ``omega`` in radians
    in (-pi, pi], IUPAC sign, and ``peptide_bond`` = |C_i - N_{i+1}| in Angstrom, stored at i.  Per row (rows,), over the bonds with at
    least one generated end: ``n_bonds`` (int32), ``max_peptide_deviation`` = max |d - 1.329| (0 without a bond), ``n_chain_break`` =
    bonds with |d - 1.329| > ``bond_tolerance``, ``n_cis`` = bonds with |omega| < pi/2.  fp64 from the fp32 points, rounded once.
    One C-ABI call; results on the device of ``designs['seq_idx']``; ValueError naming the argument before any device work."""
    who = "metrics.backbone()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    tol = _check_distance(who, "bond_tolerance", bond_tolerance)
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)
    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    pts = _hip.dev_f32(backbone_from_frames(_hip.dev_f32(designs["translations"]), _hip.dev_f32(designs["orientations"]), ("N", "CA", "C")))
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    chain, ridx = chain.to(dev), ridx.to(dev)
    per_residue = [torch.empty(rows, K, dtype=torch.float32, device=dev) for _ in range(4)]
    n_bonds, n_break, n_cis = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3))
    worst = torch.empty(rows, dtype=torch.float32, device=dev)
    nbytes = backbone_workspace_bytes(G, K)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_backbone(_hip.ptr(pts), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(chain), _hip.ptr(ridx), rows, group_size, K, tol,
                                           *[_hip.ptr(t) for t in per_residue], _hip.ptr(n_bonds), _hip.ptr(worst), _hip.ptr(n_break),
                                           _hip.ptr(n_cis), _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_backbone")
    out = dict(zip(("phi", "psi", "omega", "peptide_bond"), per_residue))
    out.update(n_bonds=n_bonds, max_peptide_deviation=worst, n_chain_break=n_break, n_cis=n_cis)
    return {k: v.to(out_dev) for k, v in out.items()}


def _frame_atoms(seq: torch.Tensor, x: torch.Tensor, O: torch.Tensor, atoms: Sequence[str]):
    """The frame atoms of residues (…,K) and their validity bits (uint8): every atom, without CB where the token is Gly."""
    pts = _hip.dev_f32(backbone_from_frames(x, O, atoms))
    bits = torch.full(seq.shape, (1 << len(atoms)) - 1, dtype=torch.uint8, device=seq.device)
    if "CB" in atoms:
        bits = torch.where(seq == GLY, bits & ~torch.tensor(1 << atoms.index("CB"), dtype=torch.uint8, device=seq.device), bits)
    return pts, bits.contiguous()


def _atom_operands(designs, generation_mask, residue_mask, context, A, atoms, group_size: int, G: int):
    """The operands every atom-level filter takes, on the device: the frame atoms ``pts`` (rows,K,P,3) of every design and their
    validity bits ``valid``; the context side ``cpts`` (G,K,A,3) / ``cvalid`` (G,K) int32 - ``context``'s real atoms (A as checked), or
    without ``context`` the frame atoms of the first row of each group (A = P); and the two masks.
    -> pts, valid, cpts, cvalid, A, gm, rm."""
    dev = _hip.device()
    seq, x, O = _hip.dev_i64(designs["seq_idx"]), _hip.dev_f32(designs["translations"]), _hip.dev_f32(designs["orientations"])
    pts, valid = _frame_atoms(seq, x, O, atoms)
    if context is None:
        first = torch.arange(G, device=dev) * group_size
        cpts, cbits = _frame_atoms(seq[first], x[first].contiguous(), O[first].contiguous(), atoms)
        A, cvalid = len(atoms), cbits.to(torch.int32).contiguous()
    else:
        cpts = _hip.dev_f32(context["xyz"])
        cvalid = _valid_word(context["atom_mask"], A, dev)
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    return pts, valid, cpts, cvalid, A, gm, rm


def contacts(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
             antigen_mask: Optional[torch.Tensor] = None, hotspot_mask: Optional[torch.Tensor] = None, chain_idx=None, residue_idx=None,
             residue_mask: Optional[torch.Tensor] = None, group_size: int = 1, clash_distance: float = 3.0, contact_distance: float = 5.0,
             atoms: Sequence[str] = BACKBONE_ATOMS) -> Dict[str, torch.Tensor]:
    """Atom clashes of the generated residues of each design, and their contacts with the antigen.  A generated residue has the frame
    atoms ``atoms`` (default N, CA, C, O, CB; no CB where the design's token is Gly) of its own row; a non-generated residue has the
    patch's real atoms, ``context['xyz']`` (G,K,A,3) where ``context['atom_mask']`` (G,K,A; bool or 0 / 1) is set, A <= 32 - ``patch.gather``'s
    output and a batch passed to ``sample()`` carry both - shared by the designs of the patch.  Without ``context`` the non-generated
    residues take the frame atoms of the first row of their group.  Eligible pairs: an atom of generated residue i and an atom of
    residue j != i, both inside ``residue_mask``, j not a chain neighbour of i (``backbone``'s rule); two generated residues count once.

    Per row (rows,): ``n_clash`` (int32) pairs closer than ``clash_distance``, ``clash_score`` = sum (clash_distance - d)^2 over them,
    ``min_distance`` (+inf without a pair).  With ``antigen_mask`` (G,K) a generated residue and a non-generated antigen residue are in
    contact when any of their atom pairs is closer than ``contact_distance``: ``n_contact_pairs``, ``n_paratope``, ``n_epitope``; with
    ``hotspot_mask`` (a subset of the antigen) ``n_hotspot_contacted`` and ``n_hotspot``.  Per residue (rows,K) int32, ready as
    ``b_factor`` of ``io.write_pdb``: ``residue_clash`` (clashing atom pairs the residue is part of, context residues included) and
    ``residue_contact`` (contact partners, on both sides; with ``antigen_mask``).  The counts are exact functions of the fp32 points
    (``include/diffab_hip.h``).  One C-ABI call; results on the device of ``designs['seq_idx']``; ValueError before any device work."""
    who = "metrics.contacts()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    atoms = _check_atoms(who, atoms)
    clash = _check_distance(who, "clash_distance", clash_distance)
    contact = _check_distance(who, "contact_distance", contact_distance)
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    if hotspot_mask is not None:
        if antigen_mask is None:
            raise ValueError(f"{who}: hotspot_mask needs an antigen_mask")
        _check_patch_mask(who, "hotspot_mask", hotspot_mask, G, K)
    A = None if context is None else _check_context(who, context, G, K)
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    P = len(atoms)
    pts, valid, cpts, cvalid, A, gm, rm = _atom_operands(designs, generation_mask, residue_mask, context, A, atoms, group_size, G)
    ag, hs = (None if m is None else _hip.dev_mask(m) for m in (antigen_mask, hotspot_mask))
    chain, ridx = chain.to(dev), ridx.to(dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = {"n_clash": i32(rows), "clash_score": torch.empty(rows, dtype=torch.float32, device=dev),
           "min_distance": torch.empty(rows, dtype=torch.float32, device=dev)}
    if ag is not None:
        out.update(n_contact_pairs=i32(rows), n_paratope=i32(rows), n_epitope=i32(rows))
    if hs is not None:
        out.update(n_hotspot_contacted=i32(rows), n_hotspot=i32(rows))
    out["residue_clash"] = i32(rows, K)
    if ag is not None:
        out["residue_contact"] = i32(rows, K)
    nbytes = contacts_workspace_bytes(G, K, A)
    ws = _hip.workspace(nbytes)
    order = ("n_clash", "clash_score", "min_distance", "n_contact_pairs", "n_paratope", "n_epitope", "n_hotspot_contacted", "n_hotspot",
             "residue_clash", "residue_contact")
    _hip.check(lib.diffab_metrics_contacts(_hip.ptr(pts), _hip.ptr(valid), _hip.ptr(cpts), _hip.ptr(cvalid), _hip.ptr(gm), _hip.ptr(rm),
                                           _hip.ptr(ag), _hip.ptr(hs), _hip.ptr(chain), _hip.ptr(ridx), rows, group_size, K, P, A, clash, contact,
                                           *[_hip.ptr(out.get(k)) for k in order], _hip.ptr(ws), nbytes, _hip.stream_ptr()),
               "diffab_metrics_contacts")
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ binding modes: contact maps and their overlap
def contact_bits_workspace_bytes(G: int, K: int, A: int) -> int:
    """DIFFAB_METRICS_CONTACT_BITS_WORKSPACE_BYTES of include/diffab_hip_interface.h."""
    return G * K * (A * 16 + 28) + G * ((K + 31) // 32 * 4 + 24) + 2048


def pairwise_bits_workspace_bytes(G: int, N: int, L: int) -> int:
    """DIFFAB_METRICS_PAIRWISE_BITS_WORKSPACE_BYTES of include/diffab_hip_interface.h."""
    Np = (N + 63) // 64 * 64
    return G * (L * Np * 4 + Np // 64 * L * 4 + L * 4 + 4) + 2048


def contact_map(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
                antigen_mask: Optional[torch.Tensor] = None, chain_idx=None, residue_idx=None, residue_mask: Optional[torch.Tensor] = None,
                group_size: int = 1, contact_distance: float = 5.0, atoms: Sequence[str] = BACKBONE_ATOMS) -> Dict[str, torch.Tensor]:
    """The contacts of each design with the antigen as data: which generated residue touches which antigen residue.  Every argument
    means what it means in ``contacts`` and is checked as there; ``antigen_mask`` (G,K) is required and K is at most 512.  Contact is
    decided by exactly the rule by which ``contacts`` counts ``n_contact_pairs`` - the same atoms (``atoms`` of the design's own frames,
    no CB where its token is Gly; ``context``'s real atoms, or the frame atoms of the first row of the group, on the antigen side), the
    same eligibility (``residue_mask``, no chain neighbours, non-generated antigen residues only) and the same fp32 comparison.

    Returns ``bits`` (rows,K,W) int32 with W = ceil(K / 32): bit ``j & 31`` of word ``j >> 5`` of row ``i`` is set iff generated residue
    i and antigen residue j are in contact, every other bit is 0; and ``n_contacts`` (rows,) int32, the number of set bits
    (= ``contacts(...)['n_contact_pairs']``).  ``unpack_contact_map`` turns the words into a bool matrix; ``pairwise_bits`` compares
    the maps of a patch's designs.  One C-ABI call (two launches, ``include/diffab_hip_interface.h``); results on the device of
    ``designs['seq_idx']``; ValueError naming the argument before any device work."""
    who = "metrics.contact_map()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    if K > INTERFACE_MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {INTERFACE_MAX_K} for a contact map")
    atoms = _check_atoms(who, atoms)
    contact = _check_distance(who, "contact_distance", contact_distance)
    if antigen_mask is None:
        raise ValueError(f"{who}: antigen_mask is required: the columns of a contact map are the antigen residues")
    _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    A = None if context is None else _check_context(who, context, G, K)
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    P = len(atoms)
    pts, valid, cpts, cvalid, A, gm, rm = _atom_operands(designs, generation_mask, residue_mask, context, A, atoms, group_size, G)
    ag = _hip.dev_mask(antigen_mask)
    chain, ridx = chain.to(dev), ridx.to(dev)
    bits = torch.empty(rows, K, (K + 31) // 32, dtype=torch.int32, device=dev)
    n_contacts = torch.empty(rows, dtype=torch.int32, device=dev)
    nbytes = contact_bits_workspace_bytes(G, K, A)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_contact_bits(_hip.ptr(pts), _hip.ptr(valid), _hip.ptr(cpts), _hip.ptr(cvalid), _hip.ptr(gm), _hip.ptr(rm),
                                               _hip.ptr(ag), _hip.ptr(chain), _hip.ptr(ridx), rows, group_size, K, P, A, contact,
                                               _hip.ptr(bits), _hip.ptr(n_contacts), _hip.ptr(ws), nbytes, _hip.stream_ptr()),
               "diffab_metrics_contact_bits")
    return {"bits": bits.to(out_dev), "n_contacts": n_contacts.to(out_dev)}


def unpack_contact_map(bits: torch.Tensor, K: int) -> torch.Tensor:
    """``contact_map``'s ``bits`` (rows,K,W) int32 -> (rows,K,K) bool: entry [r,i,j] is bit ``j & 31`` of word ``j >> 5`` of row i.
    Plain torch, for inspection and tests."""
    who = "metrics.unpack_contact_map()"
    if not _is_int(K) or K < 1:
        raise ValueError(f"{who}: K must be an int >= 1, got {K!r}")
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or bits.dim() != 3 or tuple(bits.shape[1:]) != (K, (K + 31) // 32):
        raise ValueError(f"{who}: bits must be an int32 tensor (rows, K = {K}, W = {(K + 31) // 32})")
    j = torch.arange(K, device=bits.device)
    return ((bits[:, :, j >> 5] >> (j & 31)) & 1).ne(0)


def pairwise_bits(bits: torch.Tensor, *, group_size: int) -> Dict[str, torch.Tensor]:
    """The overlap of the bit sets of the N = ``group_size`` designs of every patch, all pairs.  ``bits`` is an int32 tensor
    (G * N, ...), read as L words per design (L at most 8192) - ``contact_map``'s ``bits`` goes in as it comes out, and any other packed
    set (the epitope residues of a design, say) works the same way; all 32 bits of a word are data, the sign bit included.

    Returns ``n_set`` (G,N) int32, the popcount of each design; ``n_common`` (G,N,N) int32, |A & B|, symmetric, its diagonal ``n_set``;
    ``fcc`` (G,N,N) fp32, ``n_common[a,b] / n_set[a]``, the fraction of a's contacts that b shares (the fraction of common contacts,
    asymmetric; 1 where a's set is empty); ``jaccard`` (G,N,N) fp32, |A & B| / |A | B|, symmetric to the bit (1 where both sets are
    empty).  Each quotient is one correctly rounded fp32 division of two exact integers.  ``cluster(1 - jaccard, cutoff)`` gives the
    binding-mode families.  One C-ABI call (four launches over the live word columns only, ``include/diffab_hip_interface.h``); results
    on ``bits``' device; ValueError naming the argument before any device work."""
    who = "metrics.pairwise_bits()"
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or bits.dim() < 2:
        raise ValueError(f"{who}: bits must be an int32 tensor (G * N, ...), one row of packed words per design")
    if not _is_int(group_size) or group_size < 1:
        raise ValueError(f"{who}: group_size must be an int >= 1, got {group_size!r}")
    if group_size > MAX_GROUP:
        raise ValueError(f"{who}: group_size = {group_size}, at most {MAX_GROUP} designs per patch")
    rows, N = int(bits.shape[0]), group_size
    if rows % N != 0:
        raise ValueError(f"{who}: {rows} design rows are not a multiple of group_size = {N}")
    L = math.prod(int(v) for v in bits.shape[1:])
    if L < 1 or L > INTERFACE_MAX_WORDS:
        raise ValueError(f"{who}: bits has L = {L} words per design, outside [1, {INTERFACE_MAX_WORDS}]")
    G = rows // N
    lib = _hip.lib()
    dev, out_dev = _hip.device(), bits.device
    b = bits.detach().to(device=dev).contiguous()
    n_set = torch.empty(G, N, dtype=torch.int32, device=dev)
    n_common = torch.empty(G, N, N, dtype=torch.int32, device=dev)
    fcc, jaccard = (torch.empty(G, N, N, dtype=torch.float32, device=dev) for _ in range(2))
    nbytes = pairwise_bits_workspace_bytes(G, N, L)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_pairwise_bits(_hip.ptr(b), G, N, L, _hip.ptr(n_set), _hip.ptr(n_common), _hip.ptr(fcc), _hip.ptr(jaccard),
                                                _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_pairwise_bits")
    out = {"n_set": n_set, "n_common": n_common, "fcc": fcc, "jaccard": jaccard}
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ developability: surface patches and sequence motifs
_KD = (1.8, -4.5, -3.5, -3.5, 2.5, -3.5, -3.5, -0.4, -3.2, 4.5, 3.8, -3.9, 1.9, 2.8, -1.6, -0.8, -0.7, -0.9, -1.3, 4.2)  # AA1 order
# patches(): Kyte-Doolittle hydropathy mapped onto [1, 2], 1 + (kd + 4.5) / 9, in AA1 order; X (UNK) weighs 0
KYTE_DOOLITTLE = tuple(1.0 + (kd + 4.5) / 9.0 for kd in _KD) + (0.0,)
# patches(): D, E = -1; K, R = +1; H = +0.1 (partly protonated at neutral pH); everything else 0
RESIDUE_CHARGE = tuple({"D": -1.0, "E": -1.0, "K": 1.0, "R": 1.0, "H": 0.1}.get(c, 0.0) for c in AA1)
# liabilities(): name -> pattern of motif_masks
LIABILITY_MOTIFS = {"n_glycosylation": "N[^P][ST]", "deamidation": "N[GS]", "isomerisation": "D[GS]", "fragmentation": "DP", "cysteine": "C",
                    "methionine": "M"}


def patches_workspace_bytes(G: int, K: int) -> int:
    """DIFFAB_METRICS_PATCHES_WORKSPACE_BYTES of include/diffab_hip_develop.h."""
    return G * K * 16 + 1024


def motifs_workspace_bytes(G: int, K: int) -> int:
    """DIFFAB_METRICS_MOTIFS_WORKSPACE_BYTES of include/diffab_hip_develop.h."""
    return G * K * 4 + 1024


def _check_weight_table(who: str, name: str, table) -> torch.Tensor:
    try:
        t = torch.as_tensor(table).detach()
    except (TypeError, ValueError, RuntimeError):
        t = None
    if t is None or t.dim() != 1 or t.is_complex() or t.dtype == torch.bool or not 1 <= t.numel() <= DEVELOP_MAX_CLASSES:
        raise ValueError(f"{who}: {name} must be a sequence or 1-d tensor of 1 to {DEVELOP_MAX_CLASSES} numbers, one per token class")
    t = t.to(torch.float32)
    if not bool(torch.isfinite(t.cpu()).all()):
        raise ValueError(f"{who}: {name} must hold finite numbers")
    return t


def _residue_sites(designs, generation_mask, residue_mask, context, group_size: int):
    """One site per residue, on the device, of checked arguments -> (sites (rows,K,3) fp32, context_sites (G,K,3) fp32, tokens (rows,K)
    int32, generation_mask (G,K), residue_mask (G,K) or None).  A row's site is the CB of its own frame, the CA where its token is Gly.
    A patch's site is slot 4 of ``context['xyz']`` where ``context['atom_mask']`` has it and the token of the group's first row is not
    Gly, else slot 1 (CA), and a non-generated residue without a CA is ANDed out of ``residue_mask``; without ``context`` it is the
    site of the first row of the group.  What ``patches`` and ``interface_energy`` put their numbers on."""
    dev = _hip.device()
    seq, x, O = _hip.dev_i64(designs["seq_idx"]), _hip.dev_f32(designs["translations"]), _hip.dev_f32(designs["orientations"])
    G, K = int(generation_mask.shape[0]), int(generation_mask.shape[1])
    frame = _hip.dev_f32(backbone_from_frames(x, O, ("CA", "CB")))  # (rows,K,2,3)
    sites = torch.where((seq == GLY).unsqueeze(-1), frame[:, :, 0], frame[:, :, 1]).contiguous()
    first = torch.arange(G, device=dev) * group_size
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    if context is None:
        csites = sites[first].contiguous()
    else:
        xyz, am = _hip.dev_f32(context["xyz"]), _hip.dev_mask(context["atom_mask"])
        A = int(xyz.shape[2])
        use_cb = (am[:, :, 4] & (seq[first] != GLY)) if A > 4 else torch.zeros(G, K, dtype=torch.bool, device=dev)
        csites = torch.where(use_cb.unsqueeze(-1), xyz[:, :, min(4, A - 1)], xyz[:, :, 1]).contiguous()
        has_site = am[:, :, 1] | gm  # a non-generated residue without a CA is absent
        rm = (has_site if rm is None else rm & has_site).contiguous()
    return sites, csites, seq.to(torch.int32).contiguous(), gm, rm


def patches(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
            antigen_mask: Optional[torch.Tensor] = None, residue_mask: Optional[torch.Tensor] = None, group_size: int = 1,
            exposed: Optional[torch.Tensor] = None, hydrophobicity=KYTE_DOOLITTLE, charge=RESIDUE_CHARGE, neighbour_distance: float = 10.0,
            max_neighbours: int = 16, vicinity_distance: float = 10.0, patch_distance: float = 7.5,
            min_distance: float = 3.8) -> Dict[str, torch.Tensor]:
    """Hydrophobic and charged surface patches of the CDRs of each design and of what they sit on: the aggregation and polyspecificity
    side of developability.  The project's own restatement of the Therapeutic Antibody Profiler's PSH / PPC / PNC on ONE SITE per
    residue; no parity with that tool is claimed.  ``designs``, ``generation_mask``, ``context``, ``antigen_mask``, ``residue_mask`` and
    ``group_size`` are ``contacts``' arguments.  A generated residue's site is the CB of its own frame (``backbone_from_frames``), the CA
    where the design's token is Gly; a non-generated residue's site is slot 4 of ``context['xyz']`` where ``context['atom_mask']`` has
    it and the token is not Gly, else slot 1 (CA), and a non-generated residue without a CA is left out; without ``context`` the
    non-generated residues take the frame sites of the first row of their group.  The antigen is ignored entirely (the unbound
    antibody is what is made), so are the residues outside ``residue_mask``.

    A residue is IN SCOPE when it is generated or within ``vicinity_distance`` of a generated residue's site, and EXPOSED when it is in
    scope and has at most ``max_neighbours`` other residues within ``neighbour_distance`` - a CB-neighbour-count proxy of a surface
    whose default threshold is this project's choice, not a measured value; ``exposed`` (rows,K) bool decides instead where a caller
    knows better (``surface``'s per-residue free points, say).  Over the pairs of exposed residues closer than ``patch_distance`` the
    term is ``w_i * w_j / max(d, min_distance)**2``: ``psh`` with w = ``hydrophobicity[token]`` (default ``KYTE_DOOLITTLE``), ``ppc``
    over the pairs of two positive and ``pnc`` of two negative ``charge[token]`` (default ``RESIDUE_CHARGE``); a token outside a table
    weighs 0.  Distances are fp32 and compared strictly, the sums fp64 in a fixed order, rounded once.

    Returns, per row (rows,): ``psh``, ``ppc``, ``pnc``, ``charge_generated``, ``charge_scope`` fp32 and ``n_scope``, ``n_exposed``,
    ``n_pairs`` int32; per residue (rows,K), ready as ``b_factor`` of ``io.write_pdb``: ``residue_psh``, ``residue_ppc``,
    ``residue_pnc`` fp32, ``n_neighbours`` int32 and ``state`` uint8 (bit 0 present, bit 1 in scope, bit 2 exposed).  One C-ABI call
    (two launches, ``include/diffab_hip_develop.h``); results on the device of ``designs['seq_idx']``; ValueError naming the argument
    before any device work."""
    who = "metrics.patches()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    if K > DEVELOP_MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {DEVELOP_MAX_K}")
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    if exposed is not None and (not isinstance(exposed, torch.Tensor) or exposed.dtype != torch.bool or tuple(exposed.shape) != (rows, K)):
        raise ValueError(f"{who}: exposed must be a bool tensor {(rows, K)} (one row per design)")
    hyd, chg = _check_weight_table(who, "hydrophobicity", hydrophobicity), _check_weight_table(who, "charge", charge)
    if hyd.numel() != chg.numel():
        raise ValueError(f"{who}: hydrophobicity has {hyd.numel()} classes and charge {chg.numel()}: one table entry per token class in both")
    near = _check_distance(who, "neighbour_distance", neighbour_distance)
    vicinity = _check_distance(who, "vicinity_distance", vicinity_distance)
    patch = _check_distance(who, "patch_distance", patch_distance)
    floor = _check_positive(who, "min_distance", min_distance)
    if not _is_int(max_neighbours) or max_neighbours < 0 or max_neighbours >= 2 ** 31:
        raise ValueError(f"{who}: max_neighbours must be an int >= 0, got {max_neighbours!r}")
    if context is not None:
        A = _check_context(who, context, G, K)
        if A < 2:
            raise ValueError(f"{who}: context['xyz'] has A = {A} atoms per residue: slot 1 (CA) is needed")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    sites, csites, tokens, gm, rm = _residue_sites(designs, generation_mask, residue_mask, context, group_size)
    ag = None if antigen_mask is None else _hip.dev_mask(antigen_mask)
    ex = None if exposed is None else _hip.dev_mask(exposed)
    hyd, chg = _hip.dev_f32(hyd), _hip.dev_f32(chg)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = {"psh": f32(rows), "ppc": f32(rows), "pnc": f32(rows), "charge_generated": f32(rows), "charge_scope": f32(rows),
           "n_scope": i32(rows), "n_exposed": i32(rows), "n_pairs": i32(rows), "residue_psh": f32(rows, K), "residue_ppc": f32(rows, K),
           "residue_pnc": f32(rows, K), "n_neighbours": i32(rows, K), "state": torch.empty(rows, K, dtype=torch.uint8, device=dev)}
    nbytes = patches_workspace_bytes(G, K)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_patches(_hip.ptr(sites), _hip.ptr(csites), _hip.ptr(tokens), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(ag),
                                          _hip.ptr(ex), _hip.ptr(hyd), _hip.ptr(chg), rows, group_size, K, int(hyd.numel()), near,
                                          max_neighbours, vicinity, patch, floor, *[_hip.ptr(t) for t in out.values()], _hip.ptr(ws), nbytes,
                                          _hip.stream_ptr()), "diffab_metrics_patches")
    return {k: v.to(out_dev) for k, v in out.items()}


def motif_masks(patterns, V: int = 21) -> torch.Tensor:
    """Patterns -> the motif words of ``diffab_metrics_motifs``: an int32 tensor (M, 4) on the CPU, word p of motif m with bit v set iff
    token class v matches at position p, zero words behind the motif's end.  ``patterns`` is a pattern, a sequence of patterns or a dict
    name -> pattern (its order is kept).  A pattern is one to four positions, each a letter of ``io.AA1`` (``X`` is UNK), ``[ST]`` (any of
    the letters), ``[^P]`` (any token below ``V`` except the letters) or ``.`` (any token below ``V``); ``V`` is the number of token
    classes, 1 to 32.  ValueError for anything else, a position that matches no class below ``V`` included."""
    who = "metrics.motif_masks()"
    if not _is_int(V) or not 1 <= V <= DEVELOP_MAX_CLASSES:
        raise ValueError(f"{who}: V must be an int in [1, {DEVELOP_MAX_CLASSES}], got {V!r}")
    if isinstance(patterns, str):
        patterns = [patterns]
    elif isinstance(patterns, dict):
        patterns = list(patterns.values())
    if not isinstance(patterns, Sequence) or not 1 <= len(patterns) <= DEVELOP_MAX_MOTIFS:
        raise ValueError(f"{who}: patterns must be a pattern, or a sequence or dict of 1 to {DEVELOP_MAX_MOTIFS} patterns")
    every = (1 << V) - 1

    def letter(c: str, pat: str) -> int:
        v = AA1.find(c)
        if len(c) != 1 or v < 0:
            raise ValueError(f"{who}: pattern {pat!r}: {c!r} is no one-letter code of {AA1}")
        if v >= V:
            raise ValueError(f"{who}: pattern {pat!r}: {c!r} is token {v}, outside the V = {V} classes")
        return 1 << v

    table = []
    for pat in patterns:
        if not isinstance(pat, str):
            raise ValueError(f"{who}: a pattern must be a str, got {pat!r}")
        words, at = [], 0
        while at < len(pat):
            c = pat[at]
            if c == "[":
                end = pat.find("]", at)
                body = pat[at + 1:end] if end > 0 else ""
                negate = body.startswith("^")
                body = body[1:] if negate else body
                if end < 0 or not body:
                    raise ValueError(f"{who}: pattern {pat!r}: a class is [letters] or [^letters]")
                word = 0
                for b in body:
                    word |= letter(b, pat)
                word = every & ~word if negate else word
                at = end + 1
            elif c == ".":
                word, at = every, at + 1
            else:
                word, at = letter(c, pat), at + 1
            if word == 0:
                raise ValueError(f"{who}: pattern {pat!r}: position {len(words)} matches no token class")
            words.append(word)
        if not 1 <= len(words) <= DEVELOP_MOTIF_WORDS:
            raise ValueError(f"{who}: pattern {pat!r} has {len(words)} positions, a motif has 1 to {DEVELOP_MOTIF_WORDS}")
        table.append([w - (1 << 32) if w >= 1 << 31 else w for w in words] + [0] * (DEVELOP_MOTIF_WORDS - len(words)))
    return torch.tensor(table, dtype=torch.int32)


def liabilities(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, motifs=LIABILITY_MOTIFS, chain_idx=None, residue_idx=None,
                residue_mask: Optional[torch.Tensor] = None, group_size: int = 1, V: int = 21) -> Dict[str, torch.Tensor]:
    """Sequence liabilities of each design: motifs along the chain that do not survive production, counted where they touch the design.
    ``motifs`` is a dict name -> pattern of ``motif_masks`` (default ``LIABILITY_MOTIFS``: the N-glycosylation sequon ``N[^P][ST]``,
    deamidation ``N[GS]``, isomerisation ``D[GS]``, fragmentation ``DP``, free ``C`` and oxidisable ``M``), at most 32 of them, and ``V``
    the number of token classes.  A motif is read along the CHAIN, not along the slots: the next residue of slot i is the lowest slot
    inside ``residue_mask`` on the same chain whose ``residue_idx`` is one higher (``backbone``'s chain neighbour; ``chain_idx`` /
    ``residue_idx`` are (K,) or (G,K), default one chain and ``arange(K)``), so a numbering gap ends a motif and a patch gathered out
    of order does not.  A match is counted iff at least one of its residues is generated: the framework's own motifs are not the
    design's fault, one that the design completes is.

    Returns one int32 tensor (rows,) per motif name, its counted matches; ``n_motifs`` (rows,) int32, their sum - a ``violation`` of
    ``pareto``; and ``motif_start`` (rows,K) int32, bit m set iff a counted match of the m-th motif starts at the residue (the sign
    bit is data).  ``n_motifs`` and ``motif_start`` are therefore no motif names.  One C-ABI call (two launches,
    ``include/diffab_hip_develop.h``); results on the device of ``designs['seq_idx']``; ValueError naming the argument before any
    device work."""
    who = "metrics.liabilities()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "ca")
    if K > DEVELOP_MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {DEVELOP_MAX_K}")
    if not isinstance(motifs, dict) or not 1 <= len(motifs) <= DEVELOP_MAX_MOTIFS or not all(isinstance(n, str) for n in motifs):
        raise ValueError(f"{who}: motifs must be a dict of 1 to {DEVELOP_MAX_MOTIFS} entries name -> pattern")
    for reserved in ("n_motifs", "motif_start"):
        if reserved in motifs:
            raise ValueError(f"{who}: motifs: {reserved!r} names an output of its own and cannot name a motif")
    try:
        words = motif_masks(motifs, V)
    except ValueError as e:
        raise ValueError(f"{who}: motifs: {e}") from None
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    M = len(motifs)
    tokens = _hip.dev_i64(designs["seq_idx"]).to(torch.int32).contiguous()
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    chain, ridx = chain.to(dev), ridx.to(dev)
    host = (ctypes.c_int32 * (M * DEVELOP_MOTIF_WORDS))(*words.flatten().tolist())
    count = torch.empty(rows, M, dtype=torch.int32, device=dev)
    total = torch.empty(rows, dtype=torch.int32, device=dev)
    start = torch.empty(rows, K, dtype=torch.int32, device=dev)
    nbytes = motifs_workspace_bytes(G, K)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_motifs(_hip.ptr(tokens), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(chain), _hip.ptr(ridx),
                                         ctypes.cast(host, ctypes.c_void_p), rows, group_size, K, M, _hip.ptr(count), _hip.ptr(total),
                                         _hip.ptr(start), _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_motifs")
    out = {name: count[:, m].contiguous() for m, name in enumerate(motifs)}
    out.update(n_motifs=total, motif_start=start)
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ binding score: a distance-binned pair potential
def pair_energy_workspace_bytes(G: int, K: int) -> int:
    """DIFFAB_METRICS_PAIR_ENERGY_WORKSPACE_BYTES of include/diffab_hip_energy.h."""
    return G * K * 24 + 1024


@dataclasses.dataclass(frozen=True, eq=False)
class PairPotential:
    """A residue-level, distance-binned pair potential: ``table`` (NB,V,V), or (V,V) for one bin - anything ``torch.as_tensor`` takes,
    kept as a float32 CPU tensor (NB,V,V) - and ``bin_edges``, NB + 1 distances in Angstrom, kept as a tuple of floats.  A pair of
    residues whose sites are d apart, ``bin_edges[b] <= d < bin_edges[b + 1]``, scores ``table[b][first][second]``, the designed
    residue's token first (for two designed residues, the lower slot's): a symmetric table does not care, an asymmetric one can hold
    paratope-versus-epitope propensities.  1 <= V <= 32 token classes, 1 <= NB <= 8 bins; the edges finite, >= 0 and strictly
    ascending, and so are their float32 squares (the comparison is made on squared distances).  ValueError otherwise."""
    table: torch.Tensor
    bin_edges: tuple

    def __post_init__(self):
        who = "metrics.PairPotential()"
        try:
            t = torch.as_tensor(self.table).detach().cpu()
        except (TypeError, ValueError, RuntimeError):
            t = None
        if t is None or t.is_complex() or t.dtype == torch.bool or t.dim() not in (2, 3):
            raise ValueError(f"{who}: table must be numbers of shape (NB, V, V) or (V, V)")
        t = t.unsqueeze(0) if t.dim() == 2 else t
        NB, V = int(t.shape[0]), int(t.shape[1])
        if t.shape[2] != V or not 1 <= V <= ENERGY_MAX_CLASSES or not 1 <= NB <= ENERGY_MAX_BINS:
            raise ValueError(f"{who}: table is {tuple(t.shape)}, expected (NB, V, V) with 1 <= NB <= {ENERGY_MAX_BINS} bins and "
                             f"1 <= V <= {ENERGY_MAX_CLASSES} token classes")
        t = t.to(torch.float32).contiguous()
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{who}: table must hold numbers that are finite in float32")
        edges = self.bin_edges
        if isinstance(edges, torch.Tensor):
            edges = edges.detach().cpu().tolist() if edges.dim() == 1 else None
        if isinstance(edges, (str, bytes)) or not isinstance(edges, Sequence) or len(edges) != NB + 1 \
                or any(isinstance(e, bool) or not isinstance(e, (int, float)) for e in edges):
            raise ValueError(f"{who}: bin_edges must be NB + 1 = {NB + 1} numbers, the edges of the table's {NB} distance bins")
        edges = tuple(float(e) for e in edges)
        e32 = torch.tensor(edges, dtype=torch.float64).to(torch.float32)
        sq = e32 * e32
        if not all(math.isfinite(e) and e >= 0 for e in edges) or not bool((e32[1:] > e32[:-1]).all()):
            raise ValueError(f"{who}: bin_edges must be finite, >= 0 and strictly ascending (in float32), got {edges}")
        if not bool(torch.isfinite(sq).all()) or not bool((sq[1:] > sq[:-1]).all()):
            raise ValueError(f"{who}: the float32 squares of bin_edges must be finite and strictly ascending, got {edges}")
        object.__setattr__(self, "table", t)
        object.__setattr__(self, "bin_edges", edges)


def contact_potential(hydrophobicity=KYTE_DOOLITTLE, charge=RESIDUE_CHARGE, bin_edges=(0.0, 6.5, 9.0), bin_scale=(1.0, 0.5),
                      hydrophobic: float = 1.0, electrostatic: float = 1.0) -> PairPotential:
    """The default table of ``interface_energy``: ``E[b][a][c] = bin_scale[b] * (-hydrophobic * (h_a - 1) * (h_c - 1) + electrostatic *
    q_a * q_c)`` with h = ``hydrophobicity`` (``KYTE_DOOLITTLE``: hydropathy on [1, 2]) and q = ``charge`` (``RESIDUE_CHARGE``), so two
    hydrophobic residues in contact and two opposite charges score below zero and two like charges above; a class whose hydrophobicity
    is 0 (X) gets zero rows and columns.  Evaluated in float64, rounded to float32 once.

    THIS IS THE PROJECT'S OWN CHOICE, a placeholder so that the call works out of the box.  It is not a fitted potential and no
    predictive value is claimed for it.  Where you have a Miyazawa-Jernigan contact-energy matrix or a paratope-epitope propensity
    table, pass it as ``PairPotential(table, bin_edges)`` instead."""
    who = "metrics.contact_potential()"
    hyd, chg = _check_weight_table(who, "hydrophobicity", hydrophobicity), _check_weight_table(who, "charge", charge)
    if hyd.numel() != chg.numel():
        raise ValueError(f"{who}: hydrophobicity has {hyd.numel()} classes and charge {chg.numel()}: one table entry per token class in both")
    try:
        scale = torch.as_tensor(bin_scale, dtype=torch.float64).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        scale = None
    if scale is None or scale.dim() != 1 or not 1 <= scale.numel() <= ENERGY_MAX_BINS or not bool(torch.isfinite(scale).all()):
        raise ValueError(f"{who}: bin_scale must be 1 to {ENERGY_MAX_BINS} finite numbers, one per distance bin")
    for name, v in (("hydrophobic", hydrophobic), ("electrostatic", electrostatic)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{who}: {name} must be a finite number, got {v!r}")
    h, q = hyd.double(), chg.double()
    pair = -float(hydrophobic) * (h - 1)[:, None] * (h - 1)[None, :] + float(electrostatic) * q[:, None] * q[None, :]
    known = (hyd != 0).double()
    pair = pair * known[:, None] * known[None, :]
    try:
        return PairPotential((scale[:, None, None] * pair[None]).to(torch.float32), bin_edges)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None


def _pair_energy(lib, sites, csites, tokens, gm, rm, ag, chain, ridx, table, edges, rows, group_size, K, min_separation, substitutions):
    """One diffab_metrics_pair_energy call on device operands -> the dict of its outputs, on the library's device."""
    dev = _hip.device()
    NB, V = int(table.shape[0]), int(table.shape[1])
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = {"e_antigen": f32(rows), "e_framework": f32(rows), "e_internal": f32(rows), "n_pairs": i32(rows, 3, NB), "residue_energy": f32(rows, K),
           "residue_antigen_energy": f32(rows, K), "n_partners": i32(rows, K), "substitution": f32(rows, K, V) if substitutions else None}
    host = (ctypes.c_float * (NB + 1))(*edges)
    G = rows // group_size
    nbytes = pair_energy_workspace_bytes(G, K)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_pair_energy(_hip.ptr(sites), _hip.ptr(csites), _hip.ptr(tokens), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(ag),
                                              _hip.ptr(chain), _hip.ptr(ridx), _hip.ptr(table), ctypes.cast(host, ctypes.c_void_p), rows,
                                              group_size, K, V, NB, min_separation, *[_hip.ptr(t) for t in out.values()], _hip.ptr(ws), nbytes,
                                              _hip.stream_ptr()), "diffab_metrics_pair_energy")
    return {k: v for k, v in out.items() if v is not None}


def interface_energy(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
                     antigen_mask: Optional[torch.Tensor] = None, residue_mask: Optional[torch.Tensor] = None, chain_idx=None, residue_idx=None,
                     group_size: int = 1, potential: Optional[PairPotential] = None, min_separation: int = 3, substitutions: bool = False,
                     native: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """A binding score of each design under a residue-level, distance-binned pair potential: every designed residue against every
    residue it touches, scored by what the two residues are - the stand-in of docking and design triage for a binding energy on
    backbone frames, and with ``native`` the DiffAb paper's IMP under this potential.  No parity with Rosetta's ddG is claimed, which
    needs side chains.  ``designs``, ``generation_mask``, ``context``, ``antigen_mask``, ``residue_mask`` and ``group_size`` are
    ``patches``' arguments and the sites are ``patches``' sites: a generated residue's is the CB of its own frame, the CA where the
    design's token is Gly; a non-generated residue's is slot 4 of ``context['xyz']`` where ``context['atom_mask']`` has it and the
    token is not Gly, else slot 1 (CA), and a non-generated residue without a CA is left out; without ``context`` the non-generated
    residues take the frame sites of the first row of their group.  Unlike ``patches`` the antigen is what this call is about.

    ``potential`` is a ``PairPotential`` (default ``contact_potential()``, a placeholder of this project's own choice - read its
    docstring).  A pair of present residues, at least one of them generated, both tokens inside the table, is counted when the squared
    distance of the two sites falls into a bin, ``edge[b]**2 <= d2 < edge[b + 1]**2`` in float32, and its term is
    ``table[b][first][second]``, the generated residue's token first (of two generated residues the lower slot's).  Pairs on one chain
    whose ``residue_idx`` differ by less than ``min_separation`` are skipped - chain neighbours are always in contact and say nothing;
    ``chain_idx`` / ``residue_idx`` are (K,) or (G,K), given together or not at all (default one chain and ``arange(K)``).  The class of a
    pair: INTERNAL when both residues are generated, ANTIGEN when the other one is inside ``antigen_mask``, FRAMEWORK otherwise.

    Returns, per row (rows,): ``e_antigen``, ``e_framework``, ``e_internal`` fp32 (every pair once; fp64 sums in a fixed order, rounded
    once) and ``e_binding``, another name of ``e_antigen``; ``n_pairs`` (rows,3,NB) int32, the counted pairs per class (0 antigen, 1
    framework, 2 internal) and bin.  Per residue (rows,K), ready as ``b_factor`` of ``io.write_pdb``: ``residue_energy`` (the terms of
    every counted pair the residue is part of; for an antigen residue its pairs with the design - the epitope's hot spots),
    ``residue_antigen_energy`` (the ANTIGEN class only) and ``n_partners`` int32.  With ``substitutions=True`` also ``substitution``
    (rows,K,V): what replacing the token of a generated residue by class v would do to ``e_antigen`` with the structure held (0 at
    the residue's own token and for every residue that is not generated).

    With ``native`` - the dict ``evaluate`` takes, (G,K) - the same entry runs on the native's frames with ``group_size`` 1 and adds
    ``native_e_antigen`` (G,), ``delta`` = ``e_antigen - native_e_antigen`` of the row's patch (rows,), ``improved`` (rows,) bool =
    ``e_antigen < native_e_antigen``, one fp32 comparison, and ``imp`` (G,), the share of improved designs of each patch.  The native
    is put on the SAME site model as the designs - the CB its frame implies, not its real CB - so that the two numbers compare like
    with like.

    One C-ABI call (two launches, ``include/diffab_hip_energy.h``), two with ``native``; results on the device of
    ``designs['seq_idx']``; ValueError naming the argument before any device work."""
    who = "metrics.interface_energy()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    if K > ENERGY_MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {ENERGY_MAX_K}")
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    if potential is None:
        potential = contact_potential()
    if not isinstance(potential, PairPotential):
        raise ValueError(f"{who}: potential must be a metrics.PairPotential (or None for metrics.contact_potential()), got {type(potential).__name__}")
    if not _is_int(min_separation) or min_separation < 0 or min_separation >= 2 ** 31:
        raise ValueError(f"{who}: min_separation must be an int >= 0, got {min_separation!r}")
    if not isinstance(substitutions, bool):
        raise ValueError(f"{who}: substitutions must be a bool, got {substitutions!r}")
    if (chain_idx is None) != (residue_idx is None):
        raise ValueError(f"{who}: chain_idx and residue_idx go together, {'chain_idx' if chain_idx is None else 'residue_idx'} is missing")
    if context is not None:
        A = _check_context(who, context, G, K)
        if A < 2:
            raise ValueError(f"{who}: context['xyz'] has A = {A} atoms per residue: slot 1 (CA) is needed")
    if native is not None:
        nG, nK = _check_frames(who, "native", native, "backbone")
        if (nG, nK) != (G, K):
            raise ValueError(f"{who}: native['seq_idx'] is {(nG, nK)}, expected {(G, K)} (one row per patch)")
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    sites, csites, tokens, gm, rm = _residue_sites(designs, generation_mask, residue_mask, context, group_size)
    ag = None if antigen_mask is None else _hip.dev_mask(antigen_mask)
    chain, ridx = chain.to(dev), ridx.to(dev)
    table = _hip.dev_f32(potential.table)
    out = _pair_energy(lib, sites, csites, tokens, gm, rm, ag, chain, ridx, table, potential.bin_edges, rows, group_size, K, min_separation,
                       substitutions)
    out["e_binding"] = out["e_antigen"]
    if native is not None:
        nsites, ncsites, ntokens, _, nrm = _residue_sites(native, generation_mask, residue_mask, context, 1)
        ref = _pair_energy(lib, nsites, ncsites, ntokens, gm, nrm, ag, chain, ridx, table, potential.bin_edges, G, 1, K, min_separation, False)
        base = ref["e_antigen"]
        per_row = base.repeat_interleave(group_size)
        out["native_e_antigen"] = base
        out["delta"] = out["e_antigen"] - per_row
        out["improved"] = out["e_antigen"] < per_row
        out["imp"] = out["improved"].view(G, group_size).float().mean(1)
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ novelty: the nearest known sequence by edit distance
def edit_nearest_workspace_bytes(R: int, M: int, LM: int) -> int:
    """DIFFAB_METRICS_EDIT_NEAREST_WORKSPACE_BYTES of include/diffab_hip_novelty.h."""
    return M * ((LM + 3) // 4 * 4 + 8) + (M + NOVELTY_CHUNK - 1) // NOVELTY_CHUNK * R * 12 + 1024


@dataclasses.dataclass(frozen=True, eq=False)
class SequenceSet:
    """M sequences of their own lengths: ``tokens`` (M,L) uint8, row m holding ``lengths[m]`` tokens in ``io.AA1`` order (20 = X) and
    255 behind them, and ``lengths`` (M,) int32; L <= 256, on any device.  Tokens of 32 or more match nothing, themselves included.
    What ``sequence_set`` builds from strings and ``design_sequences`` from designs, and what ``novelty`` compares.  ValueError otherwise."""
    tokens: torch.Tensor
    lengths: torch.Tensor

    def __post_init__(self):
        who = "metrics.SequenceSet()"
        t, n = self.tokens, self.lengths
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2:
            raise ValueError(f"{who}: tokens must be a uint8 tensor (M, L)")
        if not isinstance(n, torch.Tensor) or n.dtype != torch.int32 or tuple(n.shape) != (int(t.shape[0]),):
            raise ValueError(f"{who}: lengths must be an int32 tensor ({int(t.shape[0])},), one length per row of tokens")
        if not 1 <= int(t.shape[1]) <= NOVELTY_MAX_LIBRARY:
            raise ValueError(f"{who}: tokens is {tuple(t.shape)}: L outside [1, {NOVELTY_MAX_LIBRARY}] tokens per sequence")
        if t.device != n.device:
            raise ValueError(f"{who}: tokens is on {t.device} and lengths on {n.device}")

    def __len__(self) -> int:
        return int(self.tokens.shape[0])


def sequence_set(strings) -> SequenceSet:
    """A ``SequenceSet`` on the CPU from one-letter strings in ``io.AA1`` order (X is token 20); as wide as the longest, at least 1.
    A letter outside ``io.AA1`` raises ValueError naming the string and the letter, a string longer than 256 too; no string gives M = 0."""
    who = "metrics.sequence_set()"
    if isinstance(strings, (str, bytes)) or not isinstance(strings, Sequence) or not all(isinstance(s, str) for s in strings):
        raise ValueError(f"{who}: strings must be a list of str")
    L = max([len(s) for s in strings] + [1])
    rows = []
    for i, s in enumerate(strings):
        if len(s) > NOVELTY_MAX_LIBRARY:
            raise ValueError(f"{who}: string {i} has {len(s)} letters, at most {NOVELTY_MAX_LIBRARY}")
        for c in s:
            if c not in AA1:
                raise ValueError(f"{who}: string {i} ({s!r}) has the letter {c!r}, which is not one of {AA1!r}")
        rows.append([AA1.index(c) for c in s] + [NOVELTY_PAD] * (L - len(s)))
    tokens = torch.tensor(rows, dtype=torch.uint8).view(len(strings), L)
    return SequenceSet(tokens, torch.tensor([len(s) for s in strings], dtype=torch.int32))


def sequence_strings(sequence_set: SequenceSet) -> list:
    """The inverse of ``sequence_set``: one string per sequence, a token of 21 or more as ``?``.  Lengths are read as clamped to the width."""
    if not isinstance(sequence_set, SequenceSet):
        raise ValueError("metrics.sequence_strings(): sequence_set must be a metrics.SequenceSet")
    L = int(sequence_set.tokens.shape[1])
    tokens, lengths = sequence_set.tokens.cpu().tolist(), sequence_set.lengths.cpu().tolist()
    return ["".join(AA1[t] if t < len(AA1) else "?" for t in row[:min(max(n, 0), L)]) for row, n in zip(tokens, lengths)]


def design_sequences(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, group_size: int = 1,
                     residue_mask: Optional[torch.Tensor] = None, segment_idx: Optional[torch.Tensor] = None, segment: Optional[int] = None,
                     max_length: int = NOVELTY_MAX_QUERY) -> SequenceSet:
    """The designed residues of every design row as a sequence: a ``SequenceSet`` of ``rows`` sequences, ``max_length`` wide, on the
    device of ``designs['seq_idx']``.  A residue is counted when it is inside ``generation_mask`` and ``residue_mask`` (both (G,K) bool,
    one row per patch) and, with ``segment_idx`` (G,K) integer and ``segment``, when ``segment_idx == segment`` - one CDR of several;
    the two are given together or not at all.  The tokens of the counted residues follow in slot order.  The largest count per patch
    is taken from the masks on the host before any device work (one small copy): a patch with more counted residues than
    ``max_length`` (1 .. 256; the default 64 is the widest query of ``novelty``) raises ValueError naming the patch.  One C-ABI call
    (``diffab_metrics_pack_sequences``, one launch)."""
    who = "metrics.design_sequences()"
    if not isinstance(designs, dict) or not isinstance(designs.get("seq_idx"), torch.Tensor):
        raise ValueError(f"{who}: designs must be a dict with seq_idx")
    seq = designs["seq_idx"]
    if seq.dim() != 2 or seq.is_floating_point() or seq.dtype == torch.bool:
        raise ValueError(f"{who}: designs['seq_idx'] must be an integer tensor (rows, K), got {tuple(seq.shape)} {seq.dtype}")
    rows, K = int(seq.shape[0]), int(seq.shape[1])
    if not _is_int(group_size) or group_size < 1:
        raise ValueError(f"{who}: group_size must be an int >= 1, got {group_size!r}")
    if group_size > MAX_GROUP:
        raise ValueError(f"{who}: group_size = {group_size}, at most {MAX_GROUP} designs per patch")
    if rows % group_size != 0:
        raise ValueError(f"{who}: {rows} design rows are not a multiple of group_size = {group_size}")
    if K < 1 or K > MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch outside [1, {MAX_K}]")
    G = rows // group_size
    _check_patch_mask(who, "generation_mask", generation_mask, G, K)
    if residue_mask is not None:
        _check_patch_mask(who, "residue_mask", residue_mask, G, K)
    if (segment_idx is None) != (segment is None):
        raise ValueError(f"{who}: segment_idx and segment go together, {'segment_idx' if segment_idx is None else 'segment'} is missing")
    if segment_idx is not None:
        if not isinstance(segment_idx, torch.Tensor) or segment_idx.is_floating_point() or segment_idx.dtype == torch.bool \
                or tuple(segment_idx.shape) != (G, K):
            raise ValueError(f"{who}: segment_idx must be an integer tensor {(G, K)} (one row per patch)")
        if not _is_int(segment) or not -2 ** 31 <= segment < 2 ** 31:
            raise ValueError(f"{who}: segment must be an int, got {segment!r}")
    if not _is_int(max_length) or not 1 <= max_length <= NOVELTY_MAX_LIBRARY:
        raise ValueError(f"{who}: max_length must be an int in [1, {NOVELTY_MAX_LIBRARY}], got {max_length!r}")
    counted = generation_mask.detach().cpu()
    if residue_mask is not None:
        counted = counted & residue_mask.detach().cpu()
    if segment_idx is not None:
        counted = counted & (segment_idx.detach().cpu() == segment)
    n = counted.sum(1)
    if G and int(n.max()) > max_length:
        g = int((n > max_length).nonzero()[0])
        raise ValueError(f"{who}: patch {g} has {int(n[g])} counted residues, more than max_length = {max_length}")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), seq.device
    tokens = _hip.dev_i64(seq).to(torch.int32).contiguous()
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    seg = None if segment_idx is None else _hip.dev_i64(segment_idx).to(torch.int32).contiguous()
    out = torch.empty(rows, max_length, dtype=torch.uint8, device=dev)
    length = torch.empty(rows, dtype=torch.int32, device=dev)
    _hip.check(lib.diffab_metrics_pack_sequences(_hip.ptr(tokens), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(seg), 0 if segment is None else segment,
                                                 rows, group_size, K, max_length, _hip.ptr(out), _hip.ptr(length), _hip.stream_ptr()),
               "diffab_metrics_pack_sequences")
    return SequenceSet(out.to(out_dev), length.to(out_dev))


def novelty(queries: SequenceSet, library: SequenceSet, *, radius: Optional[int] = None, exclude=None,
            matrix: bool = False) -> Dict[str, torch.Tensor]:
    """Which designs are new: for every sequence of ``queries`` (R of them, at most 64 wide) the nearest sequence of ``library`` (M of
    them, at most 256 wide) by Levenshtein distance - the least number of single-residue insertions, deletions and substitutions,
    each at cost 1, so a known loop one residue longer or a motif in another register is found, which position-by-position identity
    (``evaluate``, ``pairwise``'s ``seq_identity``) cannot.  Two residues match iff their tokens are equal and below 32; lengths
    outside their row are read as clamped.  ``exclude`` is an integer tensor (R,), the library entry each query is not compared with
    (an index outside [0, M) excludes nothing), or ``"self"`` for ``arange(R)``, which needs R == M: the set against itself.

    Returns, on the device of ``queries.tokens``, per query (R,): ``distance`` int32, the least distance; ``index`` int64, the lowest
    library entry that attains it; ``identity`` fp32 = ``1 - distance / max(length, nearest_length)`` (1 for two empty sequences);
    ``length`` and ``nearest_length`` int32, the two lengths behind it; with ``radius`` (an int) ``n_within`` int32, the library
    entries, the excluded one aside, with a distance of at most ``radius``; with ``matrix=True`` ``matrix`` (R,M) int32, every distance
    (the excluded entry's too; R * M < 2^31).  With nothing to compare (M = 0, or the only entry excluded) ``distance``, ``index`` and
    ``nearest_length`` are -1, ``identity`` is NaN and ``n_within`` is 0.

    The usual numbers.  NOVELTY of a design: ``distance > 0`` against the known set (the training set, a repertoire, disclosed
    binders); what distance makes a design "novel" is the caller's call.  UNIQUENESS among R designs:
    ``novelty(q, q, exclude="self", radius=0)["n_within"] == 0``.  FAMILIES across register shifts: the ``matrix`` of a patch's N
    designs against themselves, as ``.float().view(1, N, N)``, is a distance matrix for ``cluster``, which groups what ``seq_identity``
    keeps apart.

    One C-ABI call (``diffab_metrics_edit_nearest``, three launches, ``include/diffab_hip_novelty.h``): Myers' bit-vector algorithm,
    all integers, every output the same bits on every run.  ValueError naming the argument before any device work."""
    who = "metrics.novelty()"
    for name, s in (("queries", queries), ("library", library)):
        if not isinstance(s, SequenceSet):
            raise ValueError(f"{who}: {name} must be a metrics.SequenceSet, got {type(s).__name__}")
    R, LQ, M, LM = len(queries), int(queries.tokens.shape[1]), len(library), int(library.tokens.shape[1])
    if LQ > NOVELTY_MAX_QUERY:
        raise ValueError(f"{who}: queries is {LQ} tokens wide, at most {NOVELTY_MAX_QUERY} (the library may be {NOVELTY_MAX_LIBRARY} wide)")
    if radius is not None and (not _is_int(radius) or not -2 ** 31 <= radius < 2 ** 31):
        raise ValueError(f"{who}: radius must be an int or None, got {radius!r}")
    if not isinstance(matrix, bool):
        raise ValueError(f"{who}: matrix must be a bool, got {matrix!r}")
    if matrix and R * M >= 2 ** 31:
        raise ValueError(f"{who}: matrix of R * M = {R} * {M} elements, fewer than 2^31 are needed")
    if isinstance(exclude, str):
        if exclude != "self":
            raise ValueError(f"{who}: exclude must be an integer tensor ({R},), 'self' or None, got {exclude!r}")
        if R != M:
            raise ValueError(f"{who}: exclude='self' needs as many queries as library entries, got R = {R} and M = {M}")
        exclude = torch.arange(R, dtype=torch.int32)
    elif exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.is_floating_point() or exclude.dtype == torch.bool or tuple(exclude.shape) != (R,):
            raise ValueError(f"{who}: exclude must be an integer tensor ({R},), 'self' or None")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), queries.tokens.device
    on = lambda t: t.detach().to(dev).contiguous()
    qt, ql, lt, ll = on(queries.tokens), on(queries.lengths), on(library.tokens), on(library.lengths)
    skip = None if exclude is None else on(exclude).clamp(-1, 2 ** 31 - 1).to(torch.int32)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = {"distance": i32(R), "index": i32(R), "n_within": i32(R) if radius is not None else None,
           "identity": torch.empty(R, dtype=torch.float32, device=dev), "matrix": i32(R, M) if matrix else None}
    nbytes = edit_nearest_workspace_bytes(R, M, LM)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_edit_nearest(_hip.ptr(qt), _hip.ptr(ql), R, LQ, _hip.ptr(lt), _hip.ptr(ll), M, LM, _hip.ptr(skip),
                                               -1 if radius is None else radius, *[_hip.ptr(t) for t in out.values()], _hip.ptr(ws), nbytes,
                                               _hip.stream_ptr()), "diffab_metrics_edit_nearest")
    out = {k: v for k, v in out.items() if v is not None}
    out["index"] = out["index"].long()
    found = out["index"] >= 0
    out["length"] = ql.clamp(0, LQ)
    nearest = ll.clamp(0, LM)[out["index"].clamp(min=0)] if M else torch.zeros(R, dtype=torch.int32, device=dev)
    out["nearest_length"] = torch.where(found, nearest, torch.full_like(nearest, -1))
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ conformation: the nearest known loop by dihedral distance
def dihedral_nearest_workspace_bytes(R: int, M: int, LQ: int, LM: int, A: int) -> int:
    """DIFFAB_METRICS_DIHEDRAL_NEAREST_WORKSPACE_BYTES of include/diffab_hip_conformation.h."""
    chunks = lambda n: (n + CONFORMATION_CHUNK - 1) // CONFORMATION_CHUNK
    side = lambda n, L: (n + 15) // 16 * ((2 * A * L + 3) // 4) * 256 + n * (8 * A + 12) + chunks(n) * 260
    return side(R, LQ) + side(M, LM) + chunks(M) * R * 12 + 8192


@dataclasses.dataclass(frozen=True, eq=False)
class DihedralSet:
    """M loops of their own lengths: ``angles`` (M,L,3) fp32 in radians, phi / psi / omega of residue i of loop m at ``[m, i]``, NaN for an
    angle that does not exist (the phi of a chain's first residue) and behind the loop's length, and ``lengths`` (M,) int32; 1 <= L <= 64,
    both on one device.  What ``dihedral_set`` builds from tables and ``design_dihedrals`` from frames, and what ``conformation``
    compares.  ValueError otherwise."""
    angles: torch.Tensor
    lengths: torch.Tensor

    def __post_init__(self):
        who = "metrics.DihedralSet()"
        t, n = self.angles, self.lengths
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or int(t.shape[2]) != len(DIHEDRALS):
            raise ValueError(f"{who}: angles must be a float32 tensor (M, L, 3)")
        if not isinstance(n, torch.Tensor) or n.dtype != torch.int32 or tuple(n.shape) != (int(t.shape[0]),):
            raise ValueError(f"{who}: lengths must be an int32 tensor ({int(t.shape[0])},), one length per row of angles")
        if not 1 <= int(t.shape[1]) <= CONFORMATION_MAX_LENGTH:
            raise ValueError(f"{who}: angles is {tuple(t.shape)}: L outside [1, {CONFORMATION_MAX_LENGTH}] residues per loop")
        if t.device != n.device:
            raise ValueError(f"{who}: angles is on {t.device} and lengths on {n.device}")

    def __len__(self) -> int:
        return int(self.angles.shape[0])


def dihedral_set(loops, degrees: bool = False) -> DihedralSet:
    """A ``DihedralSet`` on the CPU from a list of loops, each an (n_i, 3) array or nested list of phi, psi, omega per residue, in radians
    or with ``degrees=True`` in degrees; ``None`` or NaN stands for an angle that does not exist.  This is how a table of canonical-class
    medians or a file of known loops comes in.  As wide as the longest loop, at least 1; a loop longer than 64 residues or not (n, 3)
    raises ValueError naming it; no loop gives M = 0."""
    who = "metrics.dihedral_set()"
    if not isinstance(degrees, bool):
        raise ValueError(f"{who}: degrees must be a bool, got {degrees!r}")
    if isinstance(loops, (str, bytes, torch.Tensor)) or not isinstance(loops, Sequence):
        raise ValueError(f"{who}: loops must be a list of (n, 3) arrays or nested lists")
    tables = []
    for i, loop in enumerate(loops):
        try:
            if isinstance(loop, torch.Tensor):
                t = loop.detach().cpu().to(torch.float64)
            else:
                rows = loop.tolist() if hasattr(loop, "tolist") else loop
                t = torch.tensor([[math.nan if v is None else float(v) for v in row] for row in rows], dtype=torch.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: loop {i} is not an (n, 3) table of numbers") from None
        if t.numel() == 0:
            t = t.reshape(0, len(DIHEDRALS))
        if t.dim() != 2 or int(t.shape[1]) != len(DIHEDRALS):
            raise ValueError(f"{who}: loop {i} is {tuple(t.shape)}, expected (n, 3): phi, psi, omega per residue")
        if int(t.shape[0]) > CONFORMATION_MAX_LENGTH:
            raise ValueError(f"{who}: loop {i} has {int(t.shape[0])} residues, at most {CONFORMATION_MAX_LENGTH}")
        tables.append(torch.deg2rad(t) if degrees else t)
    L = max([int(t.shape[0]) for t in tables] + [1])
    angles = torch.full((len(tables), L, len(DIHEDRALS)), math.nan, dtype=torch.float32)
    for m, t in enumerate(tables):
        angles[m, :int(t.shape[0])] = t.float()
    return DihedralSet(angles, torch.tensor([int(t.shape[0]) for t in tables], dtype=torch.int32))


def design_dihedrals(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, group_size: int = 1, chain_idx=None,
                     residue_idx=None, residue_mask: Optional[torch.Tensor] = None, segment_idx: Optional[torch.Tensor] = None,
                     segment: Optional[int] = None, max_length: int = CONFORMATION_MAX_LENGTH) -> DihedralSet:
    """The backbone dihedrals of the designed residues of every design row as a loop: a ``DihedralSet`` of ``rows`` loops, ``max_length``
    wide, on the device of ``designs['seq_idx']``.  The angles are those of ``backbone`` (same ``chain_idx``, ``residue_idx``,
    ``residue_mask``: NaN where the neighbour an angle needs does not exist).  A residue is counted by the rule of ``design_sequences``:
    inside ``generation_mask`` and ``residue_mask`` (both (G,K) bool, one row per patch) and, with ``segment_idx`` (G,K) integer and
    ``segment``, where ``segment_idx == segment`` - one CDR of several; the two are given together or not at all.  The angles of the
    counted residues follow in slot order.  The largest count per patch is taken from the masks on the host before any device work: a
    patch with more counted residues than ``max_length`` (1 .. 64) raises ValueError naming the patch.  It serves natives as well as
    designs: a library of known loops is ``design_dihedrals`` of their own frames, so one builder makes both sides of ``conformation``.
    Two C-ABI calls (``diffab_metrics_backbone``, then ``diffab_metrics_pack_dihedrals``, one launch)."""
    who = "metrics.design_dihedrals()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    residue_tables(who, chain_idx, residue_idx, None, G, K)
    if (segment_idx is None) != (segment is None):
        raise ValueError(f"{who}: segment_idx and segment go together, {'segment_idx' if segment_idx is None else 'segment'} is missing")
    if segment_idx is not None:
        if not isinstance(segment_idx, torch.Tensor) or segment_idx.is_floating_point() or segment_idx.dtype == torch.bool \
                or tuple(segment_idx.shape) != (G, K):
            raise ValueError(f"{who}: segment_idx must be an integer tensor {(G, K)} (one row per patch)")
        if not _is_int(segment) or not -2 ** 31 <= segment < 2 ** 31:
            raise ValueError(f"{who}: segment must be an int, got {segment!r}")
    if not _is_int(max_length) or not 1 <= max_length <= CONFORMATION_MAX_LENGTH:
        raise ValueError(f"{who}: max_length must be an int in [1, {CONFORMATION_MAX_LENGTH}], got {max_length!r}")
    counted = generation_mask.detach().cpu()
    if residue_mask is not None:
        counted = counted & residue_mask.detach().cpu()
    if segment_idx is not None:
        counted = counted & (segment_idx.detach().cpu() == segment)
    n = counted.sum(1)
    if G and int(n.max()) > max_length:
        g = int((n > max_length).nonzero()[0])
        raise ValueError(f"{who}: patch {g} has {int(n[g])} counted residues, more than max_length = {max_length}")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    bb = backbone(designs, generation_mask, chain_idx=chain_idx, residue_idx=residue_idx, residue_mask=residue_mask, group_size=group_size)
    phi, psi, omega = (_hip.dev_f32(bb[k]) for k in DIHEDRALS)
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    seg = None if segment_idx is None else _hip.dev_i64(segment_idx).to(torch.int32).contiguous()
    out = torch.empty(rows, max_length, len(DIHEDRALS), dtype=torch.float32, device=dev)
    length = torch.empty(rows, dtype=torch.int32, device=dev)
    _hip.check(lib.diffab_metrics_pack_dihedrals(_hip.ptr(phi), _hip.ptr(psi), _hip.ptr(omega), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(seg),
                                                 0 if segment is None else segment, rows, group_size, K, max_length, _hip.ptr(out),
                                                 _hip.ptr(length), _hip.stream_ptr()), "diffab_metrics_pack_dihedrals")
    return DihedralSet(out.to(out_dev), length.to(out_dev))


def dihedral_features(angles: torch.Tensor, which: Sequence[int]) -> torch.Tensor:
    """(M,L,A,2) fp32: (cos, sin) of the angle kinds ``which`` of ``angles`` (M,L,3), taken in float64 and rounded once; NaN, NaN for an
    angle that is not finite.  The operand of ``diffab_metrics_dihedral_nearest``, which takes no cosine itself."""
    a = angles[..., list(which)].double()
    return torch.stack([torch.cos(a).float(), torch.sin(a).float()], dim=-1).contiguous()


def conformation(queries: DihedralSet, library: DihedralSet, *, angles: Sequence[str] = ("phi", "psi"), radius: Optional[float] = None,
                 exclude=None, matrix: bool = False, labels: Optional[torch.Tensor] = None, min_terms: int = 1) -> Dict[str, torch.Tensor]:
    """Which designs have a known shape: for every loop of ``queries`` (R of them) the nearest loop of ``library`` (M of them) AMONG THOSE
    OF ITS OWN LENGTH by backbone-dihedral distance, d = the mean of ``2 (1 - cos(difference))`` over the compared angles - no
    superposition, no frame, blind to where the loop sits.  ``angles`` is a non-empty subset of ``DIHEDRALS`` without repeats, taken in
    ``DIHEDRALS`` order.  An angle that is NaN on either side is left out of that pair; a pair is comparable when the (clamped) lengths are
    equal and at least ``min_terms`` (>= 1) angles are compared; d is in [0, 4], and North, Lehmann and Dunbrack's D over phi and psi
    is ``2 * d``, so published cut-offs apply after halving.  ``exclude`` is an integer tensor (R,), the library entry each query is not
    compared with (an index outside [0, M) excludes nothing), or ``"self"`` for ``arange(R)``, which needs R == M.  ``labels`` is an
    integer tensor (M,), the canonical class of each library entry.

    Returns, on the device of ``queries.angles``, per query (R,): ``distance`` fp32, the least d (+inf with nothing comparable);
    ``index`` int64, the lowest library entry that attains it (-1); ``n_terms`` int32, the angles compared in that pair (0);
    ``length`` and ``nearest_length`` int32 (-1 where none); with ``radius`` (a float) ``n_within`` int32, the library entries, the
    excluded one aside, with ``d <= radius`` (0 for a negative or NaN radius); with ``matrix=True`` ``matrix`` (R,M) fp32, every d (the
    excluded entry's too; +inf for a pair that is not comparable; R * M < 2^31); with ``labels`` ``label`` int64 = ``labels[index]``, -1
    where nothing was comparable.

    The usual numbers.  The CANONICAL CLASS of every design: ``label`` where ``distance <= cutoff``.  STRUCTURAL NOVELTY:
    ``distance > cutoff`` against every known loop of that length.  FAMILIES BY SHAPE: the ``matrix`` of a patch's N designs against
    themselves, as ``.view(1, N, N)``, is a distance matrix for ``cluster`` (+inf keeps loops of other lengths apart).
    ``dihedral_angle(distance)`` reads a distance as degrees.

    One C-ABI call (``diffab_metrics_dihedral_nearest``, five launches, ``include/diffab_hip_conformation.h``); the product of the features
    runs on the fp32 matrix cores.  ValueError naming the argument before any device work."""
    who = "metrics.conformation()"
    for name, s in (("queries", queries), ("library", library)):
        if not isinstance(s, DihedralSet):
            raise ValueError(f"{who}: {name} must be a metrics.DihedralSet, got {type(s).__name__}")
    R, LQ, M, LM = len(queries), int(queries.angles.shape[1]), len(library), int(library.angles.shape[1])
    if isinstance(angles, str) or not isinstance(angles, Sequence) or len(angles) == 0 or any(a not in DIHEDRALS for a in angles) \
            or len(set(angles)) != len(angles):
        raise ValueError(f"{who}: angles must be a non-empty subset of {DIHEDRALS} without repeats, got {angles!r}")
    which = [i for i, a in enumerate(DIHEDRALS) if a in angles]
    A = len(which)
    if radius is not None and (isinstance(radius, bool) or not isinstance(radius, (int, float))):
        raise ValueError(f"{who}: radius must be a float or None, got {radius!r}")
    if not isinstance(matrix, bool):
        raise ValueError(f"{who}: matrix must be a bool, got {matrix!r}")
    if matrix and R * M >= 2 ** 31:
        raise ValueError(f"{who}: matrix of R * M = {R} * {M} elements, fewer than 2^31 are needed")
    if not _is_int(min_terms) or not 1 <= min_terms < 2 ** 31:
        raise ValueError(f"{who}: min_terms must be an int >= 1, got {min_terms!r}")
    if isinstance(exclude, str):
        if exclude != "self":
            raise ValueError(f"{who}: exclude must be an integer tensor ({R},), 'self' or None, got {exclude!r}")
        if R != M:
            raise ValueError(f"{who}: exclude='self' needs as many queries as library entries, got R = {R} and M = {M}")
        exclude = torch.arange(R, dtype=torch.int32)
    elif exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.is_floating_point() or exclude.dtype == torch.bool or tuple(exclude.shape) != (R,):
            raise ValueError(f"{who}: exclude must be an integer tensor ({R},), 'self' or None")
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.dtype == torch.bool or tuple(labels.shape) != (M,):
            raise ValueError(f"{who}: labels must be an integer tensor ({M},), one class per library entry, or None")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), queries.angles.device
    on = lambda t: t.detach().to(dev).contiguous()
    qf, lf = dihedral_features(on(queries.angles), which), dihedral_features(on(library.angles), which)
    ql, ll = on(queries.lengths), on(library.lengths)
    skip = None if exclude is None else on(exclude).clamp(-1, 2 ** 31 - 1).to(torch.int32)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {"distance": f32(R), "index": i32(R), "n_terms": i32(R), "n_within": i32(R) if radius is not None else None,
           "matrix": f32(R, M) if matrix else None}
    nbytes = dihedral_nearest_workspace_bytes(R, M, LQ, LM, A)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_dihedral_nearest(_hip.ptr(qf), _hip.ptr(ql), R, LQ, _hip.ptr(lf), _hip.ptr(ll), M, LM, A, _hip.ptr(skip),
                                                   -1.0 if radius is None else float(radius), min_terms, *[_hip.ptr(t) for t in out.values()],
                                                   _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_metrics_dihedral_nearest")
    out = {k: v for k, v in out.items() if v is not None}
    out["index"] = out["index"].long()
    found = out["index"] >= 0
    at = out["index"].clamp(min=0)
    out["length"] = ql.clamp(0, LQ)
    nearest = ll.clamp(0, LM)[at] if M else torch.zeros(R, dtype=torch.int32, device=dev)
    out["nearest_length"] = torch.where(found, nearest, torch.full_like(nearest, -1))
    if labels is not None:
        label = on(labels).long()[at] if M else torch.zeros(R, dtype=torch.int64, device=dev)
        out["label"] = torch.where(found, label, torch.full_like(label, -1))
    return {k: v.to(out_dev) for k, v in out.items()}


def dihedral_angle(distance: torch.Tensor) -> torch.Tensor:
    """``degrees(acos(1 - d / 2))`` elementwise: the angle difference that, on every compared angle, would give the distance d of
    ``conformation`` - 0 for 0, 90 for 2, 180 for 4, NaN beyond.  For reading the number; plain torch."""
    if not isinstance(distance, torch.Tensor) or not distance.is_floating_point():
        raise ValueError("metrics.dihedral_angle(): distance must be a float tensor")
    return torch.rad2deg(torch.acos(1.0 - distance / 2.0))


# ------------------------------------------------------------------ accessible and buried surface
@functools.lru_cache(maxsize=None)
def _sphere_table(n: int) -> torch.Tensor:
    golden = math.pi * (3.0 - math.sqrt(5.0))
    rows = []
    for k in range(n):
        z = 1.0 - (2 * k + 1) / n
        r = math.sqrt(1.0 - z * z)
        rows.append((r * math.cos(k * golden), r * math.sin(k * golden), z))
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def sphere_points(n: int) -> torch.Tensor:
    """(n,3) fp32 unit vectors on the golden spiral: z_k = 1 - (2k+1)/n, phi_k = k pi (3 - sqrt 5), u_k = (sqrt(1 - z_k^2) cos phi_k,
    sqrt(1 - z_k^2) sin phi_k, z_k), built in float64 and rounded to fp32.  The table ``surface`` hands the kernels."""
    if not _is_int(n) or not SURFACE_MIN_POINTS <= n <= SURFACE_MAX_POINTS:
        raise ValueError(f"metrics.sphere_points(): n must be an int in [{SURFACE_MIN_POINTS}, {SURFACE_MAX_POINTS}], got {n!r}")
    return _sphere_table(n).clone()


def surface_workspace_bytes(G: int, K: int, A: int, S: int) -> int:
    """DIFFAB_METRICS_SURFACE_WORKSPACE_BYTES of include/diffab_hip_analysis.h."""
    return G * K * (A * (16 + 16 * ((S + 63) // 64)) + 20) + G * 32 + 2048


def surface(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
            antigen_mask: Optional[torch.Tensor] = None, hotspot_mask: Optional[torch.Tensor] = None,
            residue_mask: Optional[torch.Tensor] = None, group_size: int = 1, probe: float = 1.4, n_points: int = 96,
            atoms: Sequence[str] = BACKBONE_ATOMS, atom_radius=None, context_radius: float = 1.8) -> Dict[str, torch.Tensor]:
    """Solvent-accessible surface of the generated residues and of the antigen, and the area they bury on each other (Shrake-Rupley:
    ``n_points`` points of ``sphere_points`` on every atom's sphere of radius + ``probe``; a point another atom's sphere holds is covered).
    Atoms as in ``contacts``: a generated residue has the frame atoms ``atoms`` of its own row (no CB where its token is Gly), a
    non-generated residue the patch's real atoms ``context['xyz']`` / ``context['atom_mask']``, shared by the designs of the patch -
    without ``context``, the frame atoms of the first row of its group.  Radii in Angstrom: the frame atoms take ``atom_radius`` (one
    number per name of ``atoms``, as a sequence or a dict; default the united-atom values ``ATOM_RADIUS`` - N 1.65, CA 1.87, C 1.76,
    O 1.40, CB 1.87, this project's own choice, no parity with any tool is claimed); the context atoms take ``context['atom_radius']``
    (G,K,A) where given, else the one number ``context_radius`` (``read_pdb`` keeps no element per atom slot) - or, without ``context``,
    the frame atoms' radii.  Non-generated residues are antigen where ``antigen_mask`` (G,K) is set and framework otherwise; framework
    atoms only occlude.  Chain neighbours cover like any other atom.

    A point of a generated atom is free when nothing of the antibody (the row's generated residues and the framework) covers it, bound
    when the antigen does not cover it either.  A point of an antigen atom is free when no antigen atom covers it, bound when nothing
    covers it, design-buried when only the generated residues cover it.  Returned per residue (rows,K): ``free_points`` (int32),
    ``free_area`` (fp32, A^2 = sum over atoms of points * 4 pi R^2 / n_points) - and, with ``antigen_mask``: ``bound_points``,
    ``design_buried_points``, ``bound_area``, ``design_buried_area`` and ``residue_buried`` (free - bound on a generated residue, the
    design-buried area on an antigen residue; ready as ``b_factor`` of ``io.write_pdb``); per row (rows,): ``bsa_paratope`` and
    ``bsa_epitope`` (free - bound area summed over the generated / the antigen residues), ``bsa_design_epitope`` (the design-buried
    area), ``n_paratope_buried`` (generated residues that lose a point), ``n_epitope_buried`` (antigen residues with a design-buried
    point); with ``hotspot_mask`` (a subset of the antigen) ``n_hotspot``, ``n_hotspot_buried`` and ``hotspot_buried_area``.  A row
    whose patch has no generated residue gives zeros.  Every count is an exact function of the fp32 atoms
    (``include/diffab_hip_analysis.h``).  One C-ABI call; results on the device of ``designs['seq_idx']``; ValueError before any
    device work."""
    who = "metrics.surface()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    atoms = _check_atoms(who, atoms)
    probe = _check_distance(who, "probe", probe)
    ctx_default = _check_distance(who, "context_radius", context_radius)
    if not _is_int(n_points) or not SURFACE_MIN_POINTS <= n_points <= SURFACE_MAX_POINTS:
        raise ValueError(f"{who}: n_points must be an int in [{SURFACE_MIN_POINTS}, {SURFACE_MAX_POINTS}], got {n_points!r}")
    if atom_radius is None:
        radii = [ATOM_RADIUS[a] for a in atoms]
    elif isinstance(atom_radius, dict):
        if any(a not in atom_radius for a in atoms):
            raise ValueError(f"{who}: atom_radius must give a radius for every name of atoms = {atoms}, got {sorted(atom_radius)}")
        radii = [atom_radius[a] for a in atoms]
    else:
        if isinstance(atom_radius, (str, torch.Tensor)) or not isinstance(atom_radius, Sequence) or len(atom_radius) != len(atoms):
            raise ValueError(f"{who}: atom_radius must be a dict or a sequence of {len(atoms)} numbers, one per name of atoms, got {atom_radius!r}")
        radii = list(atom_radius)
    radii = [_check_distance(who, f"atom_radius of {a}", r) for a, r in zip(atoms, radii)]
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    if hotspot_mask is not None:
        if antigen_mask is None:
            raise ValueError(f"{who}: hotspot_mask needs an antigen_mask")
        _check_patch_mask(who, "hotspot_mask", hotspot_mask, G, K)
    A = ctx_radius = None
    if context is not None:
        A = _check_context(who, context, G, K)
        ctx_radius = context.get("atom_radius")
        if ctx_radius is not None:
            if not isinstance(ctx_radius, torch.Tensor) or not ctx_radius.is_floating_point() or tuple(ctx_radius.shape) != (G, K, A):
                raise ValueError(f"{who}: context['atom_radius'] must be a float tensor {(G, K, A)}")
            if not bool(torch.isfinite(ctx_radius).all()) or bool((ctx_radius < 0).any()):
                raise ValueError(f"{who}: context['atom_radius'] must be finite and >= 0 everywhere")

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    P = len(atoms)
    pts, valid, cpts, cvalid, A, gm, rm = _atom_operands(designs, generation_mask, residue_mask, context, A, atoms, group_size, G)
    if context is None:
        crad = torch.tensor(radii, dtype=torch.float32, device=dev).expand(G, K, P).contiguous()
    else:
        crad = None if ctx_radius is None else _hip.dev_f32(ctx_radius)
    ag, hs = (None if m is None else _hip.dev_mask(m) for m in (antigen_mask, hotspot_mask))
    table = _hip.dev_f32(_sphere_table(n_points))
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {"free_points": i32(rows, K), "free_area": f32(rows, K)}
    if ag is not None:
        out.update(bound_points=i32(rows, K), design_buried_points=i32(rows, K), bound_area=f32(rows, K), design_buried_area=f32(rows, K),
                   residue_buried=f32(rows, K), bsa_paratope=f32(rows), bsa_epitope=f32(rows), bsa_design_epitope=f32(rows),
                   n_paratope_buried=i32(rows), n_epitope_buried=i32(rows))
    if hs is not None:
        out.update(n_hotspot=i32(rows), n_hotspot_buried=i32(rows), hotspot_buried_area=f32(rows))
    nbytes = surface_workspace_bytes(G, K, A, n_points)
    ws = _hip.workspace(nbytes)
    order = ("free_points", "bound_points", "design_buried_points", "free_area", "bound_area", "design_buried_area", "residue_buried",
             "bsa_paratope", "bsa_epitope", "bsa_design_epitope", "n_paratope_buried", "n_epitope_buried", "n_hotspot", "n_hotspot_buried",
             "hotspot_buried_area")
    host_radii = (ctypes.c_float * P)(*radii)
    _hip.check(lib.diffab_metrics_surface(_hip.ptr(pts), _hip.ptr(valid), host_radii, _hip.ptr(cpts), _hip.ptr(cvalid), _hip.ptr(crad),
                                          _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(ag), _hip.ptr(hs), _hip.ptr(table), rows, group_size, K, P, A,
                                          n_points, probe, ctx_default, *[_hip.ptr(out.get(k)) for k in order], _hip.ptr(ws), nbytes,
                                          _hip.stream_ptr()), "diffab_metrics_surface")
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ backbone hydrogen bonds, secondary structure
def hbonds_workspace_bytes(G: int, K: int, A: int) -> int:
    """DIFFAB_METRICS_HBONDS_WORKSPACE_BYTES of include/diffab_hip_hbonds.h."""
    return G * K * (8 + 4 * ((K + 31) // 32)) + 1024


def ss_strings(ss: torch.Tensor) -> list:
    """``hbonds()['ss']`` (rows,K) (or one row, (K,)) as one string of ``SS_LETTERS`` per row."""
    if not isinstance(ss, torch.Tensor) or ss.is_floating_point() or ss.dtype == torch.bool or ss.dim() not in (1, 2):
        raise ValueError(f"metrics.ss_strings(): ss must be an integer tensor (rows, K) or (K,) of codes 0..{len(SS_LETTERS) - 1}")
    codes = ss.detach().cpu().to(torch.int64).reshape(-1, ss.shape[-1])
    if codes.numel() and (int(codes.min()) < 0 or int(codes.max()) >= len(SS_LETTERS)):
        raise ValueError(f"metrics.ss_strings(): codes outside 0..{len(SS_LETTERS) - 1}")
    return ["".join(SS_LETTERS[c] for c in row) for row in codes.tolist()]


def hbonds(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, context: Optional[Dict[str, torch.Tensor]] = None,
           antigen_mask: Optional[torch.Tensor] = None, hotspot_mask: Optional[torch.Tensor] = None, chain_idx=None, residue_idx=None,
           residue_mask: Optional[torch.Tensor] = None, group_size: int = 1) -> Dict[str, torch.Tensor]:
    """Backbone hydrogen bonds (Kabsch-Sander's electrostatic energy, E < -0.5 kcal/mol) and the secondary structure built on them, of
    every design.  A generated residue has N, CA, C of its own row's frame; a non-generated residue the patch's real N, CA, C, O -
    slots 0..3 of ``context['xyz']`` (G,K,A,3), A >= 4, where ``context['atom_mask']`` is set, the order of ``io.read_pdb`` and
    ``patch.gather`` - shared by the designs of the patch; without ``context``, N, CA, C of the first row of its group and no real O.
    The carbonyl O the frames do not determine is built in the peptide plane from the next residue's N (at a chain end, the ideal
    placement of ``io.IDEAL_BACKBONE``), the amide H from the previous residue's C=O; a Pro token (the design's own, or for a
    non-generated residue that of the first row of the group) has no H.  Chain neighbours by ``chain_idx`` / ``residue_idx`` as in
    ``backbone``.  K <= 512.

    Per residue: ``O``, ``H`` (rows,K,3), NaN where absent - the atoms ``contacts`` and ``surface`` only approximate;
    ``nh_o_partner`` / ``nh_o_energy`` and ``o_hn_partner`` / ``o_hn_energy`` (rows,K,2), the two best bonds of the residue's N-H and of
    its C=O (-1 / 0 where fewer); ``bridge_partner`` (rows,K,2) int32 and ``bridge_parallel`` (rows,K,2) bool; ``ss`` (rows,K) uint8,
    the code of ``SS_LETTERS`` = " HBEGITS" (``ss_strings`` gives the strings); ``residue_hbonds`` (rows,K) int32, the bonds with a
    generated end the residue is part of, ready as ``b_factor`` of ``io.write_pdb``.  Per row (rows,), over the bonds with at least one
    generated end: ``n_hbonds``, ``n_hbonds_internal``, ``n_hbonds_framework``, ``hbond_energy``, ``ss_count`` (rows,8) over the
    generated residues; with ``antigen_mask`` ``n_hbonds_antigen``; with ``hotspot_mask`` ``n_hotspot_bonded`` and ``n_hotspot``.
    Every bond, partner and state is an exact function of the fp32 inputs (``include/diffab_hip_hbonds.h``; no parity with mkdssp is
    claimed: no bulge linking, I after H).  One C-ABI call; results on the device of ``designs['seq_idx']``; ValueError naming the
    argument before any device work."""
    who = "metrics.hbonds()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    if K > HBONDS_MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {HBONDS_MAX_K} (the bond matrix of a row stays on chip)")
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    if hotspot_mask is not None:
        if antigen_mask is None:
            raise ValueError(f"{who}: hotspot_mask needs an antigen_mask")
        _check_patch_mask(who, "hotspot_mask", hotspot_mask, G, K)
    A = 4
    if context is not None:
        A = _check_context(who, context, G, K)
        if A < 4:
            raise ValueError(f"{who}: context['xyz'] has A = {A} atoms per residue, N, CA, C, O (at least 4) are needed")
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    seq, x, O = _hip.dev_i64(designs["seq_idx"]), _hip.dev_f32(designs["translations"]), _hip.dev_f32(designs["orientations"])
    pts = _hip.dev_f32(backbone_from_frames(x, O, ("N", "CA", "C")))
    pro = seq.eq(PRO).contiguous()
    first = torch.arange(G, device=dev) * group_size
    cpro = pro[first].contiguous()
    if context is None:
        cpts = torch.zeros(G, K, 4, 3, dtype=torch.float32, device=dev)
        cpts[:, :, :3] = pts[first]
        cvalid = torch.full((G, K), 7, dtype=torch.int32, device=dev)
    else:
        cpts = _hip.dev_f32(context["xyz"])
        cvalid = _valid_word(context["atom_mask"], A, dev)
    gm = _hip.dev_mask(generation_mask)
    rm, ag, hs = (None if m is None else _hip.dev_mask(m) for m in (residue_mask, antigen_mask, hotspot_mask))
    chain, ridx = chain.to(dev), ridx.to(dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {"O": f32(rows, K, 3), "H": f32(rows, K, 3), "nh_o_partner": i32(rows, K, 2), "nh_o_energy": f32(rows, K, 2),
           "o_hn_partner": i32(rows, K, 2), "o_hn_energy": f32(rows, K, 2), "bridge_partner": i32(rows, K, 2),
           "bridge_parallel": torch.empty(rows, K, 2, dtype=torch.bool, device=dev), "ss": torch.empty(rows, K, dtype=torch.uint8, device=dev),
           "residue_hbonds": i32(rows, K), "n_hbonds": i32(rows), "n_hbonds_internal": i32(rows)}
    if ag is not None:
        out["n_hbonds_antigen"] = i32(rows)
    out["n_hbonds_framework"] = i32(rows)
    if hs is not None:
        out.update(n_hotspot_bonded=i32(rows), n_hotspot=i32(rows))
    out.update(hbond_energy=f32(rows), ss_count=i32(rows, 8))
    nbytes = hbonds_workspace_bytes(G, K, A)
    ws = _hip.workspace(nbytes)
    order = ("O", "H", "nh_o_partner", "nh_o_energy", "o_hn_partner", "o_hn_energy", "bridge_partner", "bridge_parallel", "ss", "residue_hbonds",
             "n_hbonds", "n_hbonds_internal", "n_hbonds_antigen", "n_hbonds_framework", "n_hotspot_bonded", "n_hotspot", "hbond_energy", "ss_count")
    _hip.check(lib.diffab_metrics_hbonds(_hip.ptr(pts), _hip.ptr(pro), _hip.ptr(cpts), _hip.ptr(cvalid), _hip.ptr(cpro), _hip.ptr(gm),
                                         _hip.ptr(rm), _hip.ptr(ag), _hip.ptr(hs), _hip.ptr(chain), _hip.ptr(ridx), rows, group_size, K, A,
                                         *[_hip.ptr(out.get(k)) for k in order], _hip.ptr(ws), nbytes, _hip.stream_ptr()),
               "diffab_metrics_hbonds")
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ design ensembles
def ensemble_workspace_bytes(G: int, N: int, K: int, P: int, V: int) -> int:
    """DIFFAB_METRICS_ENSEMBLE_WORKSPACE_BYTES of include/diffab_hip.h."""
    return G * 8 * ((N + 127) // 128 * K * (V + 3 * P + 1) + K * (V + 3 * P) + N * ((K + 63) // 64) * 3 + 1) + G * 4 * (K + 1) + 4096


def ensemble(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, group_size: int, residue_mask: Optional[torch.Tensor] = None,
             weights: Optional[torch.Tensor] = None, atoms: str = "ca", num_classes: int = 21,
             pseudocount: float = 0.0) -> Dict[str, torch.Tensor]:
    """The N = ``group_size`` designs of each patch as a distribution.  ``designs``, the masks and ``atoms`` as for ``pairwise``;
    ``weights`` (G,N) or (rows,) float, finite and >= 0 (default all ones; a negative or non-finite weight counts as 0) - for instance
    ``torch.softmax(samples['steering']['log_weight'].view(G, N), 1)`` of a steered run, or a 0 / 1 mask of the designs that passed
    ``backbone`` / ``contacts`` or belong to one cluster.  V = ``num_classes`` in [1, 32]; ``pseudocount`` a >= 0.

    Per position, at the positions inside ``residue_mask`` (elsewhere NaN / -1): ``aa_freq`` (G,K,V) = (c_v + a/V) / (W_k + a) with c_v
    the weight of the designs whose token is v (a token outside [0, V) is in no class) and W_k their sum, NaN where W_k + a = 0;
    ``entropy`` (G,K) in nats; ``consensus`` (G,K) int64, the smallest most frequent class, -1 where W_k = 0; ``mean_points``
    (G,K,P,3), the weighted mean in the patch frame (nothing is superposed), NaN where all weights are 0; ``rmsf`` (G,K) =
    sqrt(sum_r w_r sum_a |p - mean|^2 / (W P)).  Per design (rows,), over the counted positions of its patch (NaN without one):
    ``log_prob`` = the mean of ln aa_freq at the design's own tokens (-inf where that frequency is 0), ``consensus_identity``,
    ``rmsd_to_mean``.  Per patch: ``n_eff`` (G,) = W^2 / sum w^2, and ``central`` (G,) int64, the design of positive weight closest to
    the mean (lowest ``rmsd_to_mean``, ties to the lower index; -1 without one).  The definition is the comment of
    ``diffab_metrics_ensemble`` in ``include/diffab_hip.h``: fp64 sums in a fixed order, rounded once.  One C-ABI call (four launches);
    results on the device of ``designs['seq_idx']``; ValueError naming the argument before any device work."""
    who = "metrics.ensemble()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, atoms)
    N = group_size
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or not weights.is_floating_point():
            raise ValueError(f"{who}: weights must be a float tensor {(G, N)} or {(rows,)}")
        if tuple(weights.shape) not in ((G, N), (rows,)):
            raise ValueError(f"{who}: weights is {tuple(weights.shape)}, expected {(G, N)} or {(rows,)}")
    if not _is_int(num_classes) or num_classes < 1 or num_classes > MAX_CLASSES:
        raise ValueError(f"{who}: num_classes = {num_classes!r} outside [1, {MAX_CLASSES}]")
    if isinstance(pseudocount, bool) or not isinstance(pseudocount, (int, float)) or not math.isfinite(pseudocount) or pseudocount < 0:
        raise ValueError(f"{who}: pseudocount must be a finite number >= 0, got {pseudocount!r}")
    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    P, V = 1 if atoms == "ca" else len(ATOMS[atoms]), num_classes
    seq, pts = _hip.dev_i64(designs["seq_idx"]), _points(designs, atoms)
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    w = None if weights is None else _hip.dev_f32(weights).reshape(rows)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {"aa_freq": f32(G, K, V), "entropy": f32(G, K), "consensus": torch.empty(G, K, dtype=torch.int64, device=dev),
           "mean_points": f32(G, K, P, 3), "rmsf": f32(G, K), "log_prob": f32(rows), "consensus_identity": f32(rows),
           "rmsd_to_mean": f32(rows), "n_eff": f32(G), "central": torch.empty(G, dtype=torch.int64, device=dev)}
    nbytes = ensemble_workspace_bytes(G, N, K, P, V)
    ws = _hip.workspace(nbytes)
    _hip.check(lib.diffab_metrics_ensemble(_hip.ptr(seq), _hip.ptr(pts), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(w), G, N, K, P, V, float(pseudocount),
                                           *[_hip.ptr(t) for t in out.values()], _hip.ptr(ws), nbytes, _hip.stream_ptr()),
               "diffab_metrics_ensemble")
    return {k: v.to(out_dev) for k, v in out.items()}


# ------------------------------------------------------------------ design similarity
def _check_positive(who: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")
    return float(v)


def similarity(designs: Dict[str, torch.Tensor], native: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, group_size: int = 1,
               atoms: str = "ca", residue_mask: Optional[torch.Tensor] = None, antigen_mask: Optional[torch.Tensor] = None,
               segment_idx: Optional[torch.Tensor] = None, num_segments: Optional[int] = None, chain_idx=None, residue_idx=None,
               inclusion_radius: float = 15.0, contact_distance: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Each design against the native of its patch without a superposition: lDDT and the recovery of the native residue contacts.
    ``designs``, the masks, ``group_size``, ``atoms`` and ``segment_idx`` / ``num_segments`` as for ``evaluate``; ``native`` holds the
    patch's own ``translations`` (and ``orientations`` for the backbone), one row per patch (G,K,...) - or one per design row, the batch
    ``sample()`` ran on, of which the first row of every group is read.  A residue is present inside ``residue_mask`` and counted when
    it is also generated.  K * P <= 1024 points per patch (K <= 256 with the backbone).

    lDDT (thresholds 0.5, 1, 2, 4 A): for a point of a counted residue i and a point of a present residue j != i, the pair is scored when
    its native distance is below ``inclusion_radius`` and preserved at a threshold when the design's distance differs by less.
    ``n_pairs`` (G,K) int32, ``preserved`` (rows,K,4) int32, ``lddt_residue`` (rows,K) (NaN where nothing is scored or the residue is not
    counted), ``lddt`` (rows,), ``lddt_thresholds`` (rows,4); with ``segment_idx`` ``lddt_segment`` (rows,S); with ``antigen_mask`` (G,K)
    the same over the pairs whose j is an antigen residue: ``n_pairs_interface``, ``preserved_interface``, ``ilddt_residue``, ``ilddt``.

    Native contacts: a counted residue i and a present partner j != i - an antigen residue with ``antigen_mask``, else a residue not
    bonded to i (|i - j| > 1 by position, or ``guidance``'s bonded rule when ``chain_idx`` / ``residue_idx``, (K,) or (G,K), are given) - are in contact
    when their closest points are nearer than ``contact_distance`` (default 8 A for ``'ca'``, 5 A for ``'backbone'``).  ``n_native`` (G,),
    ``native_contacts_residue`` (G,K), ``n_design``, ``n_kept`` (rows,) int32, ``fnat`` = n_kept / n_native, ``fnonnat`` = (n_design -
    n_kept) / n_design (NaN on a zero denominator) and ``kept_residue`` (rows,K) int32, ready as ``b_factor`` of ``io.write_pdb``.

    The counts are exact functions of the fp32 points and every ratio is one fp32 division of two of them (``include/diffab_hip.h``).
    One C-ABI call, one launch, no workspace; results on the device of ``designs['seq_idx']``; ValueError before any device work."""
    who = "metrics.similarity()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, atoms)
    if not isinstance(native, dict) or not isinstance(native.get("translations"), torch.Tensor):
        raise ValueError(f"{who}: native must be a dict with translations (and orientations for atoms='backbone')")
    nx = native["translations"]
    if not nx.is_floating_point() or nx.dim() != 3 or tuple(nx.shape[1:]) != (K, 3) or int(nx.shape[0]) not in (G, rows):
        raise ValueError(f"{who}: native['translations'] is {tuple(nx.shape)} {nx.dtype}, expected a float tensor {(G, K, 3)} or {(rows, K, 3)}")
    nR = int(nx.shape[0])
    if atoms == "backbone":
        nO = native.get("orientations")
        if not isinstance(nO, torch.Tensor) or not nO.is_floating_point() or tuple(nO.shape) != (nR, K, 3, 3):
            raise ValueError(f"{who}: native['orientations'] must be a float tensor {(nR, K, 3, 3)} for atoms='backbone'")
    P = 1 if atoms == "ca" else len(ATOMS[atoms])
    if K * P > SIMILARITY_MAX_POINTS:
        raise ValueError(f"{who}: K * P = {K} * {P} points per patch, at most {SIMILARITY_MAX_POINTS} are staged on chip")
    if antigen_mask is not None:
        _check_patch_mask(who, "antigen_mask", antigen_mask, G, K)
    S = 0
    if segment_idx is not None:
        if not isinstance(segment_idx, torch.Tensor) or segment_idx.is_floating_point() or segment_idx.dtype == torch.bool:
            raise ValueError(f"{who}: segment_idx must be an integer tensor")
        if tuple(segment_idx.shape) != (G, K):
            raise ValueError(f"{who}: segment_idx is {tuple(segment_idx.shape)}, expected {(G, K)}")
        if num_segments is None:
            num_segments = max(1, int(segment_idx.max()) + 1) if segment_idx.numel() else 1
        if not _is_int(num_segments) or num_segments < 1 or num_segments > MAX_SEGMENTS:
            raise ValueError(f"{who}: num_segments = {num_segments!r} (segment_idx labels up to it) outside [1, {MAX_SEGMENTS}]")
        S = num_segments
    elif num_segments is not None:
        raise ValueError(f"{who}: num_segments without segment_idx")
    radius = _check_positive(who, "inclusion_radius", inclusion_radius)
    cutoff = _check_positive(who, "contact_distance", CONTACT_DISTANCE[atoms] if contact_distance is None else contact_distance)
    chain = ridx = None
    if chain_idx is not None or residue_idx is not None:  # (checked, and unused with an antigen_mask: the partners are the antigen residues)
        chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)

    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    pts = _points(designs, atoms)
    first = None if nR == G else torch.arange(G) * group_size  # a native per design row: the first row of every group
    npts = _points({k: (v if first is None else v[first.to(v.device)]) for k, v in native.items()
                    if k in ("translations", "orientations") and isinstance(v, torch.Tensor)}, atoms)
    gm = _hip.dev_mask(generation_mask)
    rm, ag = (None if m is None else _hip.dev_mask(m) for m in (residue_mask, antigen_mask))
    seg = None if segment_idx is None else _hip.dev_i64(segment_idx)
    if chain is not None:
        chain, ridx = chain.to(dev), ridx.to(dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    with_ag, with_seg = ag is not None, S > 0
    out = {"n_pairs": i32(G, K), "n_pairs_interface": i32(G, K) if with_ag else None, "preserved": i32(rows, K, 4),
           "preserved_interface": i32(rows, K, 4) if with_ag else None, "lddt_residue": f32(rows, K), "lddt": f32(rows),
           "lddt_thresholds": f32(rows, 4), "ilddt_residue": f32(rows, K) if with_ag else None, "ilddt": f32(rows) if with_ag else None,
           "lddt_segment": f32(rows, S) if with_seg else None, "n_native": i32(G), "native_contacts_residue": i32(G, K),
           "n_design": i32(rows), "n_kept": i32(rows), "fnat": f32(rows), "fnonnat": f32(rows), "kept_residue": i32(rows, K)}
    _hip.check(lib.diffab_metrics_similarity(_hip.ptr(pts), _hip.ptr(npts), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(ag), _hip.ptr(seg), _hip.ptr(chain),
                                             _hip.ptr(ridx), rows, group_size, K, P, S, radius, cutoff, *[_hip.ptr(t) for t in out.values()],
                                             _hip.stream_ptr()), "diffab_metrics_similarity")
    return {k: v.to(out_dev) for k, v in out.items() if v is not None}
