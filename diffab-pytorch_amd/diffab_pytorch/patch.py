"""Patch construction from a whole complex on the device: which K residues of an
N-residue antibody-antigen complex the sampler sees, the reference batch fields at patch size, and the designs pasted back into the
complex.  The reference cuts its patches in ``preprocess_pdb.py:44-58`` with ``protstruc`` (the nearest-k residues around the CDR
anchor residues, united with the nearest-k antigen residues, then ``residue_masked_select``); ``protstruc`` is not in the reference
tree, so the selection follows this project's own four-step definition (``include/diffab_hip.h``: ``diffab_patch_select``) and parity
with ``protstruc.get_cdr_anchor_mask`` / ``get_topk_nearest_residue_mask`` is UNPINNED, as for ``features.featurize``.

``select`` -> ``gather`` -> ``DiffAb.sample`` -> ``paste`` is ``DiffAb.design_complex``.  Every step runs on the HIP kernels of
``csrc/patch_kernels.hip``; there is no torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional

import torch

from . import _hip

CA_IDX = 1  # atom slot of CA in (B,N,A,3) coordinates, as features.featurize
MAX_RESIDUES = 4096  # DIFFAB_PATCH_MAX_RESIDUES: residues per complex the selection kernel holds

# the per-residue fields of the reference batch dict plus the ones this package adds (io.read_pdb, sample(allowed_aa=...))
PER_RESIDUE_FIELDS = ("seq_idx", "xyz", "orientations", "backbone_dihedrals", "backbone_dihedrals_mask", "atom_mask", "chain_idx",
                      "residue_idx", "residue_mask", "generation_mask", "antigen_mask", "anchor_mask", "allowed_aa", "resseq", "icode")
PAIR_FIELDS = ("distmat", "pairwise_dihedrals")


class PatchIndex(NamedTuple):
    """``index`` (B,K) int64: the residues of each patch in ascending order, -1 in the unused slots; ``mask`` (B,K) bool: true on the
    first ``count`` slots; ``count`` (B,) int32."""
    index: torch.Tensor
    mask: torch.Tensor
    count: torch.Tensor


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_mask(who: str, name: str, m, B: int, N: int) -> None:
    if not isinstance(m, torch.Tensor) or m.dtype != torch.bool:
        raise ValueError(f"{who}: {name} must be a bool tensor")
    if tuple(m.shape) != (B, N):
        raise ValueError(f"{who}: {name} is {tuple(m.shape)}, expected {(B, N)}")


def select(xyz: torch.Tensor, generation_mask: torch.Tensor, *, k: int = 128, k_antigen: Optional[int] = None,
           antigen_mask: Optional[torch.Tensor] = None, anchor_mask: Optional[torch.Tensor] = None,
           chain_idx: Optional[torch.Tensor] = None, residue_mask: Optional[torch.Tensor] = None, pad_to: int = 128) -> PatchIndex:
    """The patch of each of B complexes of N residues (padded; ``residue_mask`` false on the padding).  ``xyz`` is (B,N,3) CA
    coordinates or (B,N,A,3) atoms with CA in slot 1.  Per complex (``diffab_patch_select``): the anchors are the residues flanking
    each generated segment on its chain (or ``anchor_mask``; the generated residues themselves when there is none); every present
    residue is keyed by its squared CA distance to the nearest anchor in fp32, generated residues and anchors first; the patch is the
    first ``k`` residues by (key, index) united with the first ``k_antigen`` residues of ``antigen_mask``, returned in ascending
    residue index.  ``k_antigen=None`` means 128 with an ``antigen_mask`` and 0 without one; the patch has K = ``k + k_antigen``
    rounded up to a multiple of ``pad_to`` rows.  A complex without a generated residue gets count 0.  One C-ABI call; the results
    live on xyz's device.

    Raises ValueError before any device work for shapes that do not match, non-bool masks, a chain_idx that is not an integer tensor,
    ``k < 1``, ``k_antigen < 0``, ``k_antigen > 0`` without ``antigen_mask``, ``pad_to < 1`` and N above ``MAX_RESIDUES``; and, after
    the call, for a complex whose generated residues and anchors alone exceed ``k`` (the kernel reports it as count -1)."""
    who = "patch.select()"
    if not isinstance(xyz, torch.Tensor) or not xyz.is_floating_point() or xyz.dim() not in (3, 4) or xyz.shape[-1] != 3:
        raise ValueError(f"{who}: xyz must be a float tensor (B, N, 3) or (B, N, A, 3)")
    if xyz.dim() == 4 and xyz.shape[2] <= CA_IDX:
        raise ValueError(f"{who}: xyz (B, N, A, 3) needs the CA slot: A >= {CA_IDX + 1}")
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    _check_mask(who, "generation_mask", generation_mask, B, N)
    for name, m in (("antigen_mask", antigen_mask), ("anchor_mask", anchor_mask), ("residue_mask", residue_mask)):
        if m is not None:
            _check_mask(who, name, m, B, N)
    if chain_idx is not None:
        if not isinstance(chain_idx, torch.Tensor) or chain_idx.is_floating_point() or chain_idx.dtype == torch.bool:
            raise ValueError(f"{who}: chain_idx must be an integer tensor")
        if tuple(chain_idx.shape) != (B, N):
            raise ValueError(f"{who}: chain_idx is {tuple(chain_idx.shape)}, expected {(B, N)}")
    if not _is_int(k) or k < 1:
        raise ValueError(f"{who}: k must be an int >= 1, got {k!r}")
    if k_antigen is None:
        k_antigen = 128 if antigen_mask is not None else 0
    if not _is_int(k_antigen) or k_antigen < 0:
        raise ValueError(f"{who}: k_antigen must be an int >= 0, got {k_antigen!r}")
    if k_antigen > 0 and antigen_mask is None:
        raise ValueError(f"{who}: k_antigen = {k_antigen} needs an antigen_mask")
    if not _is_int(pad_to) or pad_to < 1:
        raise ValueError(f"{who}: pad_to must be an int >= 1, got {pad_to!r}")
    if N > MAX_RESIDUES:
        raise ValueError(f"{who}: N = {N} residues per complex, the selection kernel holds at most {MAX_RESIDUES}")
    K = -(-(k + k_antigen) // pad_to) * pad_to

    lib = _hip.lib()
    x = _hip.dev_f32(xyz)
    dev = x.device
    stride = 3 if x.dim() == 3 else 3 * int(x.shape[2])
    ca_ptr = C.c_void_p(x.data_ptr() + (0 if x.dim() == 3 else 4 * 3 * CA_IDX)) if x.numel() else C.c_void_p(0)
    gm = _hip.dev_mask(generation_mask)
    rm, am, ag = (None if m is None else _hip.dev_mask(m) for m in (residue_mask, anchor_mask, antigen_mask))
    ch = None if chain_idx is None else _hip.dev_i64(chain_idx)
    index = torch.empty(B, K, dtype=torch.int64, device=dev)
    mask = torch.empty(B, K, dtype=torch.bool, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    _hip.check(lib.diffab_patch_select(ca_ptr, stride, _hip.ptr(rm), _hip.ptr(gm), _hip.ptr(am), _hip.ptr(ch), _hip.ptr(ag), B, N, k,
                                       k_antigen, K, _hip.ptr(index), _hip.ptr(mask), _hip.ptr(count), _hip.stream_ptr()),
               "diffab_patch_select")
    bad = (count.cpu() < 0).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"{who}: complex {bad[0]} has more generated and anchor residues than k = {k} (they are always in the patch)"
                         + (f"; so have complexes {bad[1:]}" if len(bad) > 1 else ""))
    out = xyz.device
    return PatchIndex(index.to(out), mask.to(out), count.to(out))


def _check_patch(who: str, patch) -> None:
    if not isinstance(patch, PatchIndex):
        raise ValueError(f"{who}: patch must be the PatchIndex that patch.select() returned, got {type(patch).__name__}")
    idx, m, c = patch
    if idx.dim() != 2 or idx.dtype != torch.int64 or m.dtype != torch.bool or tuple(m.shape) != tuple(idx.shape) or \
            tuple(c.shape) != (idx.shape[0],):
        raise ValueError(f"{who}: malformed PatchIndex (index {tuple(idx.shape)} {idx.dtype}, mask {tuple(m.shape)} {m.dtype}, "
                         f"count {tuple(c.shape)})")


def _complex_size(who: str, batch, B: int) -> int:
    if not isinstance(batch, dict):
        raise ValueError(f"{who}: batch must be a dict of the reference's batch fields")
    for name in ("seq_idx", "xyz"):
        if name not in batch:
            raise ValueError(f"{who}: the batch has no {name!r}")
    N = int(batch["seq_idx"].shape[1]) if batch["seq_idx"].dim() == 2 else -1
    for name in PER_RESIDUE_FIELDS:
        v = batch.get(name)
        if v is None:
            continue
        lead = (1, N) if name == "residue_idx" and v.dim() == 2 and v.shape[0] == 1 else (B, N)
        if not isinstance(v, torch.Tensor) or v.dim() < 2 or tuple(v.shape[:2]) != lead:
            raise ValueError(f"{who}: {name} is {tuple(getattr(v, 'shape', ()))}, expected ({B}, {N}, ...) like the patch index and seq_idx")
    return N


def _gather_rows(lib, src: torch.Tensor, index: torch.Tensor, complex_of_row=None) -> torch.Tensor:
    """src (B,N,...) on the device, contiguous; index (rows,K) on the device -> (rows,K,...)."""
    B, N = int(src.shape[0]), int(src.shape[1])
    rows, K = int(index.shape[0]), int(index.shape[1])
    if src.numel() == 0:  # a field without bytes per residue
        return src.new_zeros((rows, K) + tuple(src.shape[2:]))
    row_bytes = src[0, 0].numel() * src.element_size()
    dst = torch.empty((rows, K) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    cor = None if complex_of_row is None else (C.c_int32 * rows)(*complex_of_row)
    _hip.check(lib.diffab_patch_gather(_hip.ptr(src), _hip.ptr(index), cor, B, N, rows, K, row_bytes, _hip.ptr(dst), _hip.stream_ptr()),
               "diffab_patch_gather")
    return dst


def gather(batch: Dict[str, torch.Tensor], patch: PatchIndex) -> Dict[str, torch.Tensor]:
    """The per-residue fields of the reference batch dict at patch size: every key of ``PER_RESIDUE_FIELDS`` that the
    batch holds, (B,N,...) -> (B,K,...), one ``diffab_patch_gather`` call per field (B rows: ``sample(num_samples=N)`` replicates the
    state on the device itself).  ``residue_idx`` ((B,N) or the reference's (1,N)) defaults to ``arange(N)`` of the COMPLEX before it
    is gathered, so the patch carries the complex's residue numbers, gaps included - what the relative-position feature of
    PairEmbedding and the chain-bond term of guidance need.  ``residue_mask`` is the gathered mask AND ``patch.mask``.  Unused slots
    (index -1) are zero in every field: chain_idx 0 is the reference's padding chain, the masks are false there.

    The pair fields (``distmat``, ``pairwise_dihedrals``) are dropped: they are (N,N) per complex, and ``sample()`` recomputes them
    from ``xyz`` on the device.  Keys outside ``PER_RESIDUE_FIELDS`` are left out.  Results live on the device of ``batch['seq_idx']``.
    ValueError before any device work for a patch that is no PatchIndex and for fields whose leading shape is not (B,N)."""
    who = "patch.gather()"
    _check_patch(who, patch)
    B = int(patch.index.shape[0])
    N = _complex_size(who, batch, B)
    lib = _hip.lib()
    dev = _hip.device()
    out_dev = batch["seq_idx"].device
    index = _hip.dev_i64(patch.index)
    out: Dict[str, torch.Tensor] = {}
    fields = dict(batch)
    if fields.get("residue_idx") is None:
        fields["residue_idx"] = torch.arange(N, device=dev).unsqueeze(0)
    for name in PER_RESIDUE_FIELDS:
        v = fields.get(name)
        if v is None:
            continue
        src = v.detach().to(dev)
        if name == "residue_idx":
            src = src.expand(B, N)
        out[name] = _gather_rows(lib, src.contiguous(), index)
    pm = patch.mask.to(dev)
    out["residue_mask"] = out["residue_mask"] & pm if "residue_mask" in out else pm.clone()
    return {k: v.to(out_dev) for k, v in out.items()}


def _complex_of_row(who: str, B: int, rows: int, num_samples, context_index) -> list:
    if not _is_int(num_samples) or num_samples < 1:
        raise ValueError(f"{who}: num_samples must be an int >= 1, got {num_samples!r}")
    if context_index is not None:
        if num_samples != 1:
            raise ValueError(f"{who}: give num_samples or context_index, not both")
        ci = torch.as_tensor(context_index)
        if ci.dim() != 1 or ci.is_floating_point() or ci.dtype == torch.bool or ci.numel() != rows:
            raise ValueError(f"{who}: context_index must be a 1-D integer tensor with one entry per design row ({rows})")
        cor = [int(v) for v in ci.tolist()]
        if any(c < 0 or c >= B for c in cor):
            raise ValueError(f"{who}: context_index names a complex outside [0, {B})")
        return cor
    if rows != B * num_samples:
        raise ValueError(f"{who}: {rows} design rows for {B} complexes x num_samples = {num_samples}")
    return [r // num_samples for r in range(rows)]


def paste(batch: Dict[str, torch.Tensor], patch: PatchIndex, samples: Dict[str, torch.Tensor], *, num_samples: int = 1,
          context_index=None) -> Dict[str, torch.Tensor]:
    """The designs at full length: ``seq_idx`` (rows,N), ``translations`` (rows,N,3) and ``orientations`` (rows,N,3,3) per design row
    of ``samples`` (``DiffAb.sample``'s result on the gathered patch) - the native complex everywhere except the generated residues of
    the patch, which take the design (``diffab_patch_scatter`` with the gathered ``generation_mask`` as the write mask).  Row r belongs
    to complex ``r // num_samples``, or ``context_index[r]``.  The native translations are the CA of ``batch['xyz']``; the batch needs
    ``orientations``.  ValueError before any device work for a malformed patch, a row count that does not match and missing fields."""
    who = "patch.paste()"
    _check_patch(who, patch)
    B, K = int(patch.index.shape[0]), int(patch.index.shape[1])
    N = _complex_size(who, batch, B)
    for name in ("orientations", "generation_mask"):
        if batch.get(name) is None:
            raise ValueError(f"{who}: the batch has no {name!r}")
    if not isinstance(samples, dict) or any(samples.get(n) is None for n in ("seq_idx", "translations", "orientations")):
        raise ValueError(f"{who}: samples must hold seq_idx, translations and orientations (DiffAb.sample's result)")
    rows = int(samples["seq_idx"].shape[0])
    for name, tail in (("seq_idx", ()), ("translations", (3,)), ("orientations", (3, 3))):
        if tuple(samples[name].shape) != (rows, K) + tail:
            raise ValueError(f"{who}: samples[{name!r}] is {tuple(samples[name].shape)}, expected {(rows, K) + tail}")
    cor = _complex_of_row(who, B, rows, num_samples, context_index)
    lib = _hip.lib()
    dev = _hip.device()
    out_dev = samples["seq_idx"].device
    xyz = batch["xyz"]
    native = {"seq_idx": _hip.dev_i64(batch["seq_idx"]), "translations": _hip.dev_f32(xyz[:, :, CA_IDX] if xyz.dim() == 4 else xyz),
              "orientations": _hip.dev_f32(batch["orientations"])}
    rows_of = torch.tensor(cor, dtype=torch.int64, device=dev)
    index = _hip.dev_i64(patch.index).index_select(0, rows_of)
    write = _gather_rows(lib, _hip.dev_mask(batch["generation_mask"]), index, cor)  # false on the -1 slots: gather zero-fills them
    out = {}
    for name, full in native.items():
        dst = full.index_select(0, rows_of)  # one copy of the native complex per design row
        src = samples[name].detach().to(device=dev, dtype=full.dtype).contiguous()
        row_bytes = src[0, 0].numel() * src.element_size()
        _hip.check(lib.diffab_patch_scatter(_hip.ptr(src), _hip.ptr(index), _hip.ptr(write), rows, N, K, row_bytes, _hip.ptr(dst),
                                            _hip.stream_ptr()), "diffab_patch_scatter")
        out[name] = dst.to(out_dev)
    return out
