"""The library's own device scratch (csrc/stream_scratch.h) under more streams than any of the tables it replaced had slots (4, 8, 16,
32), and under growth: every stream computes the same bytes, a captured graph keeps computing them after the buffers it was captured
with have been outgrown and after the other streams have been through, and hip.workspace retires what it outgrows.  Each stream that
runs a deferred reduction owns a 1 GiB split-K arena and a 128 MiB LayerNorm arena for the rest of the process, so the module uses 36
streams and no more."""
import pytest
import torch

from speecht5_amd import hip

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_TN = hip.A_KSTRIDED | hip.B_KSTRIDED | hip.OUT_F32
N_STREAMS = 34            # test 1, and the churn of test 2: one more than the largest table that was (32), and one to spare


@pytest.fixture(scope="module")
def streams(cuda):
    """36 torch streams with 36 distinct handles, of both priorities (torch hands out streams from a pool per priority)."""
    made = [torch.cuda.Stream(device=cuda, priority=p) for p in (0, -1) for _ in range(N_STREAMS)]
    by_handle = {}
    for s in made:
        by_handle.setdefault(s.cuda_stream, s)
    by_handle.pop(torch.cuda.default_stream(cuda).cuda_stream, None)
    assert len(by_handle) >= N_STREAMS + 2, f"{len(by_handle)} distinct stream handles"
    return list(by_handle.values())[:N_STREAMS + 2]


def _inputs(cuda, fill_cols=80, sc_rows=200, sc_cols=64, gemm=(256, 256, 4096)):
    """One fixed seed; the split-K shape and flags are test_layer_exit_gpu.test_splitk_tn_gate's (nsplit > 1)."""
    g = torch.Generator().manual_seed(11)
    M, N, K = gemm
    i = {
        "fill_dx": torch.randn(300, fill_cols, generator=g).to(BF), "fill_mask": (torch.rand(300, generator=g) < 0.4).to(torch.uint8),
        "fill_dv": torch.randn(fill_cols, generator=g),
        "sc_dy": torch.randn(sc_rows, sc_cols, generator=g).to(BF), "sc_tok": torch.randint(0, 50, (sc_rows,), generator=g, dtype=torch.int32),
        "sc_table": torch.randn(50, sc_cols, generator=g),
        "sq32": torch.randn(5000, generator=g), "sq16": torch.randn(5000, generator=g).to(BF),
        "A": (torch.randn(K, M, generator=g) * 0.25).to(BF), "B": (torch.randn(K, N, generator=g) * 0.25).to(BF),
        "C": torch.randn(M, N, generator=g), "asum": torch.randn(M, generator=g),
        "ln_x": (torch.randn(64, 256, generator=g) * 2 + 0.5).to(BF), "ln_dy": torch.randn(64, 256, generator=g).to(BF),
        "ln_g": torch.randn(256, generator=g), "ln_b": torch.randn(256, generator=g),
        "ln_dg": torch.randn(256, generator=g), "ln_db": torch.randn(256, generator=g),
    }
    i = {k: v.to(cuda) for k, v in i.items()}
    i["ln_mean"], i["ln_rstd"] = torch.empty(64, device=cuda), torch.empty(64, device=cuda)
    y = torch.empty_like(i["ln_x"])
    hip.check(hip.lib().st5_layernorm_fwd(i["ln_x"].data_ptr(), i["ln_g"].data_ptr(), i["ln_b"].data_ptr(), y.data_ptr(), i["ln_mean"].data_ptr(),
                                          i["ln_rstd"].data_ptr(), 64, 256, 1e-5, hip.BF16, hip.stream()), "st5_layernorm_fwd")
    i["gemm"] = gemm
    torch.cuda.synchronize()
    return i


def _outputs(i):
    """The tensors _ops writes: allocated once, reset by _ops itself (so a captured _ops can be replayed)."""
    o = {k: torch.empty_like(i[k]) for k in ("fill_dx", "fill_dv", "sc_table")}
    o["sq32"], o["sq16"] = torch.empty(1, device=i["C"].device), torch.empty(1, device=i["C"].device)
    for tag in ("imm", "def"):
        o["C_" + tag], o["asum_" + tag] = torch.empty_like(i["C"]), torch.empty_like(i["asum"])
        o["ln_dx_" + tag], o["ln_dg_" + tag], o["ln_db_" + tag] = torch.empty_like(i["ln_x"]), torch.empty_like(i["ln_dg"]), torch.empty_like(i["ln_db"])
    return o


def _fill(i, o, st):
    o["fill_dx"].copy_(i["fill_dx"]); o["fill_dv"].copy_(i["fill_dv"])
    rows, cols = i["fill_dx"].shape
    hip.check(hip.lib().st5_masked_fill_rows_bwd(o["fill_dx"].data_ptr(), i["fill_mask"].data_ptr(), o["fill_dv"].data_ptr(), rows, cols, hip.BF16, st),
              "st5_masked_fill_rows_bwd")


def _scatter(i, o, st):
    o["sc_table"].copy_(i["sc_table"])
    rows, cols = i["sc_dy"].shape
    hip.check(hip.lib().st5_embed_rows_bwd_det_w(i["sc_dy"].data_ptr(), i["sc_tok"].data_ptr(), o["sc_table"].data_ptr(), rows, cols, 50, 0.5, None, 1, 1,
                                                 hip.BF16, st), "st5_embed_rows_bwd_det_w")


def _gemm(i, o, tag):
    M, N, K = i["gemm"]
    o["C_" + tag].copy_(i["C"]); o["asum_" + tag].copy_(i["asum"])
    hip.gemm(hip.operand(i["A"], M), hip.operand(i["B"], N), hip.operand(o["C_" + tag], N), M, N, K, hip.BF16, flags=_TN | hip.DEFERRABLE, beta=1.0,
             asum=o["asum_" + tag])


def _ln_bwd(i, o, tag, st):
    L = hip.lib()
    o["ln_dg_" + tag].copy_(i["ln_dg"]); o["ln_db_" + tag].copy_(i["ln_db"])
    ws = hip.workspace(L.st5_layernorm_bwd_ws_bytes(64, 256), i["ln_x"].device)
    hip.check(L.st5_layernorm_bwd(i["ln_dy"].data_ptr(), i["ln_x"].data_ptr(), i["ln_g"].data_ptr(), i["ln_mean"].data_ptr(), i["ln_rstd"].data_ptr(),
                                  o["ln_dx_" + tag].data_ptr(), o["ln_dg_" + tag].data_ptr(), o["ln_db_" + tag].data_ptr(), ws.data_ptr(), 64, 256,
                                  None, 0.0, 0, hip.BF16, st), "st5_layernorm_bwd")


def _ops(i, o):
    """All six scratch sites on the current stream: fill backward, scatter, st5_sumsq (fp32, bf16), split-K GEMM and LayerNorm backward
    with the immediate reductions, then both again with the deferred ones."""
    L, st = hip.lib(), hip.stream()
    _fill(i, o, st)
    _scatter(i, o, st)
    hip.check(L.st5_sumsq(i["sq32"].data_ptr(), o["sq32"].data_ptr(), 5000, 1.0, 0, hip.F32, st), "st5_sumsq")
    hip.check(L.st5_sumsq(i["sq16"].data_ptr(), o["sq16"].data_ptr(), 5000, 1.0, 0, hip.BF16, st), "st5_sumsq")
    _gemm(i, o, "imm")
    _ln_bwd(i, o, "imm", st)
    hip.check(L.st5_gemm_defer_splitk(1, st), "st5_gemm_defer_splitk")
    hip.check(L.st5_layernorm_defer(1, st), "st5_layernorm_defer")
    try:
        _gemm(i, o, "def")
        _ln_bwd(i, o, "def", st)
        hip.check(L.st5_gemm_flush_splitk(st), "st5_gemm_flush_splitk")
        hip.check(L.st5_layernorm_flush(st), "st5_layernorm_flush")
    finally:
        hip.check(L.st5_layernorm_defer(0, st), "st5_layernorm_defer")
        hip.check(L.st5_gemm_defer_splitk(0, st), "st5_gemm_defer_splitk")


def _snap(o):
    torch.cuda.synchronize()
    return {k: v.cpu().contiguous().view(-1).view(torch.uint8) for k, v in o.items()}


def _run_on(s, i, o):
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _ops(i, o)
    return _snap(o)


def _differs(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_every_stream_computes_the_same_bytes_twice_round(cuda, streams):
    i = _inputs(cuda)
    o = _outputs(i)
    assert len({s.cuda_stream for s in streams[:N_STREAMS]}) == N_STREAMS >= 33
    first = _run_on(streams[0], i, o)
    # the ops ran: accumulators moved off their initial values, the sums are the sums
    init = {"fill_dv": i["fill_dv"], "sc_table": i["sc_table"], "C_imm": i["C"], "asum_def": i["asum"], "ln_dg_imm": i["ln_dg"], "ln_db_def": i["ln_db"]}
    for k, v in init.items():
        assert not torch.equal(first[k], v.cpu().view(-1).view(torch.uint8)), k
    assert abs(float(o["sq32"]) - float(i["sq32"].double().pow(2).sum())) < 1e-3 * 5000
    assert abs(float(o["sq16"]) - float(i["sq16"].double().pow(2).sum())) < 1e-3 * 5000
    for tag in ("C", "asum", "ln_dx", "ln_dg", "ln_db"):      # immediate == deferred reduction
        assert torch.equal(first[tag + "_imm"], first[tag + "_def"]), tag
    for rnd in range(2):
        for n, s in enumerate(streams[:N_STREAMS]):
            assert _differs(first, _run_on(s, i, o)) == [], (rnd, n)


def test_captured_graph_survives_growth_and_churn(cuda, streams):
    i = _inputs(cuda)
    o = _outputs(i)
    A, fresh, others = streams[N_STREAMS], streams[N_STREAMS + 1], streams[:N_STREAMS]
    assert len({s.cuda_stream for s in others} - {A.cuda_stream, fresh.cuda_stream}) >= 33
    _run_on(A, i, o)                                        # warm-up: first use of every buffer, outside capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=A, capture_error_mode="thread_local"):
        _ops(i, o)
    graph.replay()
    first = _snap(o)
    # Eagerly on A, past each floor, so that the buffers the graph was captured with are superseded:
    #   fill partials   256 x 4096 floats = 4 MiB                 (had 256 x 80 floats)
    #   scatter         20000 rows x 2048 cols: 20000 * 8 B of indices + 2 * 625 * 2048 floats = 9.9 MiB   (floor 8 MiB)
    #   split-K slabs   256 x 768 x 22016: 3 tiles of 256^2, 86 splits x 256 x 768 floats = 64.5 MiB        (floor 64 MiB; grows to 128 MiB)
    big = _inputs(cuda, fill_cols=4096, sc_rows=20000, sc_cols=2048, gemm=(256, 768, 22016))
    ob = _outputs(big)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        st = hip.stream()
        _fill(big, ob, st)
        _scatter(big, ob, st)
        _gemm(big, ob, "imm")
    torch.cuda.synchronize()
    assert not torch.isnan(ob["C_imm"]).any() and not torch.equal(ob["C_imm"], big["C"])
    o2 = _outputs(i)
    for s in others:                                        # ... and every other stream goes through all six sites
        assert _differs(first, _run_on(s, i, o2)) == []
    for v in o.values():
        v.fill_(float("nan")) if v.is_floating_point() else v.zero_()
    graph.replay()
    again = _snap(o)
    assert _differs(first, again) == []
    assert _differs(first, _run_on(fresh, i, o2)) == []


def test_workspace_retires_what_it_outgrows(cuda, streams):
    with torch.cuda.stream(streams[N_STREAMS + 1]):
        b1 = hip.workspace(1, cuda)
        n1 = b1.numel()
        assert hip.workspace(n1, cuda) is b1
        b2 = hip.workspace(2 * n1, cuda)
        assert b2.data_ptr() != b1.data_ptr() and b2.numel() == max(2 * n1, 1 << 20)
        assert any(t is b1 for t in hip._ws_retired)
        assert hip.workspace(n1, cuda) is b2 and hip.workspace(1, cuda) is b2
        b3 = hip.workspace(2 * n1 + 1, cuda)              # growth at least doubles: retired stays below current
        assert b3.numel() == 4 * n1 and any(t is b2 for t in hip._ws_retired)
        assert sum(t.numel() for t in (b1, b2)) < b3.numel()
