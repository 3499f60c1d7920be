"""The patch-resident module launch hands to_out's output tile to the next layer's projections through LDS (K = 128) and writes it to
global memory for the last layer only.  The seams where that hand-over starts and ends - the first layer (input rows staged from global
memory), the last (output written for the heads and the caller) - at NL = 1, 2 and 3, against the per-layer launches that keep the
global hand-over: equal bit for bit, at a batch whose last round of patches is partly filled (264 patches: some work-groups walk two)."""
import pytest
import torch

import diffab_oracle as orc
from diffab_pytorch import DiffAb, _hip, synthetic as syn
from sampler_support import hip

pytestmark = pytest.mark.gpu


def _model(NL):
    d = dict(syn.BENCH_DIMS, NL=NL)
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], T=100).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(d, seed=NL, prefix=""))
    return d, model


def _patches(B, K, dims, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {
        "res_context_emb": torch.randn(B, K, dims["D"], device="cuda", generator=g),
        "pair_context_emb": torch.randn(B, K, K, dims["C"], device="cuda", generator=g),
        "translations": 10 * torch.randn(B, K, 3, device="cuda", generator=g),
        "seq_idx": torch.randint(0, 20, (B, K), device="cuda", generator=g),
    }
    out["orientations"] = orc.uniform_rotation_from_normals(torch.randn(B, K, 4, device="cuda", generator=g).cpu()).cuda()
    start = torch.randint(0, K - 20, (B, 1), device="cuda", generator=g)
    pos = torch.arange(K, device="cuda")[None]
    out["generation_mask"] = (pos >= start) & (pos < start + 12)
    return out


@pytest.mark.parametrize("NL", [1, 2, 3])
@pytest.mark.parametrize("B", [8, 264])
def test_module_launch_lds_handover_is_bitwise_the_per_layer_launches(hip, NL, B):
    dims, model = _model(NL)
    inp = _patches(B, 128, dims, seed=100 * NL + B)
    kw = dict(res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"], generation_mask=inp["generation_mask"],
              seed=3, t_stop=97)
    a = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], flags=_hip.FLAG_PERSISTENT_MODULE, **kw)
    b = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], flags=_hip.FLAG_MULTI_LAUNCH, **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), (NL, B, k)
    gm = inp["generation_mask"]
    assert not torch.equal(a["translations"][gm], inp["translations"][gm])
    del inp
    torch.cuda.empty_cache()
