"""The numpy restatement of diffab_metrics_pair_energy (include/diffab_hip_energy.h), shared by
test_pair_energy_host.py and test_gpu_pair_energy.py.  Not a test module: importing it loads no library and touches no device.

The squared distances and every comparison are numpy float32, grouped as the header fixes them (test_geometry_host.d2_f32), so the
integers are what the kernel must EQUAL; a term is one float32 table entry, exact in float64, and every sum is float64 over the SAME
float32 sites and tables, rounded to float32 once at the end.  Beside every float output the restatement returns the sum of |term|
behind it under sum_abs[name], the scale of the error an fp64 sum in another order may carry."""
import numpy as np

from developability_ref import same_bits  # noqa: F401 (the GPU tests take it from here)
from test_geometry_host import d2_f32

f32 = np.float32
ANTIGEN, FRAMEWORK, INTERNAL = 0, 1, 2
FLOATS = ("e_antigen", "e_framework", "e_internal", "residue_energy", "residue_antigen_energy", "substitution")
INTS = ("n_pairs", "n_partners")


def pair_energy_ref(sites, context_sites, tokens, gen, rm=None, antigen=None, chain=None, ridx=None, *, table, bin_edges, group_size=1,
                    min_separation=3, substitutions=True):
    """sites (rows,K,3) fp32, context_sites (G,K,3) fp32, tokens (rows,K) int, gen / rm / antigen (G,K) bool, chain / ridx (G,K) int
    (both or neither), table (NB,V,V) fp32, bin_edges NB + 1 numbers -> dict of the outputs of diffab_metrics_pair_energy, the float
    ones as float32 plus their float64 values under '<name>_f64', and 'sum_abs': {name: float64 array of the output's shape}."""
    sites, context_sites = np.asarray(sites, f32), np.asarray(context_sites, f32)
    table = np.asarray(table, f32)
    table = table[None] if table.ndim == 2 else table
    NB, V = table.shape[:2]
    t64 = table.astype(np.float64)
    edges = np.asarray(bin_edges, f32)
    assert edges.shape == (NB + 1,) and (chain is None) == (ridx is None)
    e2 = edges * edges
    rows, K = tokens.shape
    out = {k: np.zeros(rows, np.float64) for k in ("e_antigen", "e_framework", "e_internal")}
    out.update({k: np.zeros((rows, K), np.float64) for k in ("residue_energy", "residue_antigen_energy")})
    out.update(n_pairs=np.zeros((rows, 3, NB), np.int32), n_partners=np.zeros((rows, K), np.int32))
    if substitutions:
        out["substitution"] = np.zeros((rows, K, V), np.float64)
    sum_abs = {k: np.zeros_like(v) for k, v in out.items() if v.dtype == np.float64}
    eye, slot = np.eye(K, dtype=bool), np.arange(K)
    for r in range(rows):
        g = r // group_size
        present = np.ones(K, bool) if rm is None else np.asarray(rm[g], bool)
        generated = np.asarray(gen[g], bool) & present
        ag = present & ~generated & (np.zeros(K, bool) if antigen is None else np.asarray(antigen[g], bool))
        xyz = np.where(generated[:, None], sites[r], context_sites[g])
        tok = np.asarray(tokens[r]).astype(np.int64)
        known = (tok >= 0) & (tok < V)
        t = np.where(known, tok, 0)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = d2_f32(xyz, xyz)
            bins = np.full((K, K), -1)
            for b in range(NB):
                bins[(d2 >= e2[b]) & (d2 < e2[b + 1])] = b
        skipped = np.zeros((K, K), bool)
        if chain is not None:
            c, n = np.asarray(chain[g]), np.asarray(ridx[g]).astype(np.int64)
            skipped = (c[:, None] == c[None, :]) & (np.abs(n[:, None] - n[None, :]) < min_separation)
        geometric = present[:, None] & present[None, :] & known[None, :] & (bins >= 0) & ~skipped & ~eye  # (what the scan asks of j)
        counted = geometric & known[:, None] & (generated[:, None] | generated[None, :])
        internal = counted & generated[:, None] & generated[None, :]
        to_antigen = counted & ~internal & (ag[:, None] | ag[None, :])
        framework = counted & ~internal & ~to_antigen
        i_first = generated[:, None] & (~generated[None, :] | (slot[:, None] < slot[None, :]))  # the generated one; of two the lower slot
        first, second = np.where(i_first, t[:, None], t[None, :]), np.where(i_first, t[None, :], t[:, None])
        b0 = np.maximum(bins, 0)
        term = np.where(counted, t64[b0, first, second], 0.0)
        assert np.array_equal(term, term.T) and np.array_equal(counted, counted.T)
        upper = np.triu(np.ones((K, K), bool), 1)
        for name, cls, which in (("e_antigen", ANTIGEN, to_antigen), ("e_framework", FRAMEWORK, framework), ("e_internal", INTERNAL, internal)):
            out[name][r] = term[which & upper].sum()
            sum_abs[name][r] = np.abs(term[which & upper]).sum()
            for b in range(NB):
                out["n_pairs"][r, cls, b] = (which & upper & (bins == b)).sum()
        out["residue_energy"][r], sum_abs["residue_energy"][r] = term.sum(1), np.abs(term).sum(1)
        out["residue_antigen_energy"][r] = np.where(to_antigen, term, 0.0).sum(1)
        sum_abs["residue_antigen_energy"][r] = np.where(to_antigen, np.abs(term), 0.0).sum(1)
        out["n_partners"][r] = counted.sum(1)
        if substitutions:
            for i in np.flatnonzero(generated):
                js = np.flatnonzero(geometric[i] & ag)
                S = t64[bins[i, js], :, t[js]].sum(0) if len(js) else np.zeros(V)  # (V,): S_v over the antigen partners
                A = np.abs(t64[bins[i, js], :, t[js]]).sum(0) if len(js) else np.zeros(V)
                cur, cur_abs = (S[tok[i]], A[tok[i]]) if known[i] else (0.0, 0.0)
                out["substitution"][r, i], sum_abs["substitution"][r, i] = S - cur, A + cur_abs
    for k in [k for k, v in out.items() if v.dtype == np.float64]:
        out[k + "_f64"] = out[k]
        out[k] = out[k].astype(f32)
    out["sum_abs"] = sum_abs
    return out


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal number below it)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), float(np.finfo(f32).tiny)).astype(f32)
    return np.spacing(x).astype(np.float64)


def bound(ref64, sum_abs):
    """|got - ref| allowed for a float output: one fp32 rounding (and the double-rounding boundary), plus what an fp64 sum of at most
    2^18 terms in another order - twice for the scan's difference of two sums - may differ by: 2^-34 * sum |term|."""
    return ulp32(ref64) + 2.0 ** -34 * np.asarray(sum_abs, np.float64)
