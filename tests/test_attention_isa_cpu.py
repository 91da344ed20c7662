"""Build check on the compiled ISA of the fused-attention kernels (no GPU): registers, scratch, occupancy of every fa2:: kernel, and
the two shapes of waste DESIGN.md section 7 removed from fa2::bwd_dkv_kernel -- one exec-mask region per score (the predicated
bucket-gradient stores and the SLOW mask tests) and one full dropout pair hash per score (the lanes of a key pair hashed the same word).
tools/attn_isa_counts.py compiles csrc/flash_attn2.hip with the flags of tools/barrier_audit.py and counts per kernel."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts():
    spec = importlib.util.spec_from_file_location("attn_isa_counts", os.path.join(ROOT, "tools", "attn_isa_counts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    c = m.kernel_counts(m.compile_to_asm())
    dem = m.demangle(list(c))
    return {re.sub(r"\(.*$", "", dem[n]).replace("void ", ""): v for n, v in c.items()}


def test_every_attention_kernel_fits_its_register_budget(counts):
    fa2 = {k: v for k, v in counts.items() if k.startswith("fa2::")}
    assert len(fa2) >= 15, sorted(fa2)
    for name, c in fa2.items():
        assert c["vgprs"] is not None and c["vgprs"] <= 256, (name, c)
        assert c["scratch"] == 0, (name, c)
    # the kernels declared __launch_bounds__(256, 2): two blocks per CU is what their LDS budget and latency hiding are sized for
    two = [k for k in fa2 if re.match(r"fa2::(fwd_kernel|bwd_dq_kernel|bwd_dkv_kernel)<", k)]
    assert len(two) == 12, two
    for name in two:
        assert fa2[name]["occupancy"] >= 2, (name, fa2[name])


@pytest.mark.parametrize("variant", ["<true, true>", "<true, false>"])
def test_dkv_bias_variant_has_no_exec_mask_region_per_score(counts, variant):
    c = counts["fa2::bwd_dkv_kernel" + variant]
    assert c["v_exp_f32"] > 0
    assert c["saveexec"] < c["v_exp_f32"], c


@pytest.mark.parametrize("variant", ["<true, true>", "<false, true>"])
def test_dkv_dropout_variant_hashes_once_per_key_pair(counts, variant):
    """v_mul_u32_u24 per score evaluated (two multiplies per pair hash): no larger than the dq kernel's ratio, which shares pair hashes
    by construction (a lane holds four adjacent keys of a row), plus 0.1 for the block key's three multiplies outside the element loop."""
    dkv, dq = counts["fa2::bwd_dkv_kernel" + variant], counts["fa2::bwd_dq_kernel" + variant]
    assert dkv["v_exp_f32"] > 0 and dq["v_exp_f32"] > 0
    assert dkv["v_mul_u32_u24"] / dkv["v_exp_f32"] <= dq["v_mul_u32_u24"] / dq["v_exp_f32"] + 0.1, (dkv, dq)
