"""The per-row step launches of the synthesis stream against their scalar forms run once per distinct position: row b of the per-row
launch is bit-equal to row b of the scalar launch at step pos[b] (st5_gemm_skinny_rows, st5_lm_decode_attn_rows,
st5_decode_cross_attn_rows, st5_tts_pe_add_rows, st5_tts_step_tail_rows), and st5_tts_rows_admit resets exactly the admitted rows.
Canary values lie on both sides of every slot and record buffer; out-of-range positions (-1, cap) are clamped or not written."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
CAP, S, H, HD = 6, 5, 2, 64
GUARD = 4096
CANARY = -7.0


def _positions(rows, cap=CAP):
    """Position sets with 0, cap - 1, two equal ones and the out-of-range -1 and cap; at 33 rows all of them in one set, cycling so
    that the rows of the second 32-row chunk differ from the rows at the same offset of the first."""
    if rows == 3:
        return [[0, cap - 1, 2], [-1, cap, 3], [4, 4, 1]]
    return [[(5 * i + 3) % (cap + 2) - 1 for i in range(rows)]]


def _clamp(p, cap):
    return min(max(p, 0), cap - 1)


def _guarded(shape, dtype, cuda, fill=CANARY):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=cuda)      # guards and buffer: ONE allocation
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _guards_intact(whole, n, fill=CANARY):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _i32(v, cuda):
    return torch.tensor(v, dtype=torch.int32, device=cuda)


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


# ---- skinny GEMM with step_rows ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", [(256, 128), (1536, 768)])      # K|V of C = 128 (one k slice) and of Base (slices and the combine kernel)
@pytest.mark.parametrize("rows", [3, 33])
def test_gemm_rows_slot_write_is_bit_equal_per_row(cuda, rows, N, K, dtype):
    from speecht5_amd import functional as Fn
    g = torch.Generator().manual_seed(rows + N)
    x = torch.randn(rows, K, generator=g).to(dtype).to(cuda)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(cuda)
    b = torch.randn(N, generator=g).to(cuda)
    n = rows * CAP * N
    kw = dict(step_stride=N, step_cap=CAP, out_ld=CAP * N)
    for pos in _positions(rows):
        ref = {}
        for p in sorted(set(pos)):
            _, buf = _guarded((rows, CAP, N), dtype, cuda)
            Fn.linear_skinny(x, w, b, out=buf, step=_i32([p], cuda), **kw)
            ref[p] = buf
        whole, buf = _guarded((rows, CAP, N), dtype, cuda)
        pos_d = _i32(pos, cuda)
        Fn.linear_skinny_rows(x, w, b, out=buf, step_rows=pos_d, **kw)
        torch.cuda.synchronize()
        assert _guards_intact(whole, n), "a guard was written"
        assert pos_d.tolist() == pos
        for r_, p in enumerate(pos):
            slot = _clamp(p, CAP)
            assert torch.equal(buf[r_, slot], ref[p][r_, slot]), (r_, p)
            rest = torch.cat([buf[r_, :slot], buf[r_, slot + 1:]])
            assert bool((rest == CANARY).all()), f"row {r_}: another slot was written"


def test_gemm_rows_requires_the_positions(cuda):
    from speecht5_amd import hip
    x = torch.zeros(4, 64, device=cuda)
    w = torch.zeros(64, 64, device=cuda)
    out = torch.zeros(4, 4, 64, device=cuda)
    rc = hip.lib().st5_gemm_skinny_rows(x.data_ptr(), 64, w.data_ptr(), 64, 0, 0, 0, out.data_ptr(), 256, 4, 64, 64, 0, 0.0, 0, 0, 0, 0, 64, 4,
                                        0, hip.F32, hip.stream())
    assert rc == 1


# ---- self-attention ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cap", [CAP, 300])                     # 300: positions on both sides of the key-range split (64)
@pytest.mark.parametrize("rows", [3, 33])
def test_self_attention_rows_is_bit_equal_per_row(cuda, rows, cap, dtype):
    from speecht5_amd import functional as Fn
    C = H * HD
    g = torch.Generator().manual_seed(rows + cap)
    q = torch.randn(rows, C, generator=g).to(dtype).to(cuda)
    kv = torch.randn(rows, cap, 2 * C, generator=g).to(dtype).to(cuda)
    anc = torch.arange(rows, dtype=torch.int32, device=cuda).unsqueeze(1).expand(rows, cap).contiguous()
    ws = Fn.lm_decode_attn_ws(rows, cap, H, HD, cuda)
    if cap == CAP:
        sets = _positions(rows)
    else:
        base = [0, 63, 64, 299, 65, 65, -1, 300, 150, 17, 128]
        sets = [base[:3], base[3:6], base[6:9]] if rows == 3 else [[base[(3 * i + i // 32) % len(base)] for i in range(rows)]]
    for pos in sets:
        ref = {}
        for p in sorted(set(pos)):
            ctx = torch.empty(rows, C, dtype=dtype, device=cuda)
            ref[p] = Fn.lm_decode_attn_dev(q, kv, anc, _i32([p], cuda), 1, cap, H, HD, ctx, ws).clone()
        whole, ctx = _guarded((rows, C), dtype, cuda)
        Fn.lm_decode_attn_rows(q, kv, anc, _i32(pos, cuda), 1, cap, H, HD, ctx, ws)
        torch.cuda.synchronize()
        assert _guards_intact(whole, rows * C)
        for r_, p in enumerate(pos):
            assert torch.equal(ctx[r_], ref[p][r_]), (r_, p)
        assert bool(torch.isfinite(ctx.float()).all())


# ---- cross-attention record column ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S_", [S, 100])                        # 100: the key range is split over workgroups and combined
@pytest.mark.parametrize("rows", [3, 33])
def test_cross_attention_rows_record_column_per_row(cuda, rows, S_, dtype):
    from speecht5_amd import functional as Fn
    C = H * HD
    g = torch.Generator().manual_seed(rows + S_)
    q = torch.randn(rows, C, generator=g).to(dtype).to(cuda)
    kv = torch.randn(rows * S_, 2 * C, generator=g).to(dtype).to(cuda)
    lens = [1 + (3 * b + 2) % S_ for b in range(rows)]          # a different key-padding mask per row
    kpm = (torch.arange(S_)[None, :] >= torch.tensor(lens)[:, None]).to(torch.uint8).to(cuda)
    ws = Fn.decode_cross_attn_ws(rows, S_, H, HD, cuda)
    n = rows * H * CAP * S_
    for pos in _positions(rows):
        ref = {}
        for p in sorted(set(pos)):
            _, rec = _guarded((rows, H, CAP, S_), torch.float32, cuda)
            ctx = torch.empty(rows, C, dtype=dtype, device=cuda)
            Fn.decode_cross_attn_step(q, kv, 0, S_, H, HD, ctx, _i32([p], cuda), CAP, kpm=kpm, rec=rec, ws=ws)
            ref[p] = (ctx, rec)
        whole, rec = _guarded((rows, H, CAP, S_), torch.float32, cuda)
        ctx = torch.empty(rows, C, dtype=dtype, device=cuda)
        Fn.decode_cross_attn_rows(q, kv, 0, S_, H, HD, ctx, _i32(pos, cuda), CAP, kpm=kpm, rec=rec, ws=ws)
        torch.cuda.synchronize()
        assert _guards_intact(whole, n), "a guard of the record was written"
        for r_, p in enumerate(pos):
            col = _clamp(p, CAP)
            assert torch.equal(ctx[r_], ref[p][0][r_]), (r_, p)
            assert torch.equal(rec[r_, :, col], ref[p][1][r_, :, col]), (r_, p)
            assert bool((rec[r_, :, col, lens[r_]:] == 0).all()) and abs(float(rec[r_, 0, col].sum()) - 1) < 1e-4
            rest = torch.cat([rec[r_, :, :col], rec[r_, :, col + 1:]], dim=1)
            assert bool((rest == CANARY).all()), f"row {r_}: another record column was written"


# ---- positional row ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [3, 33])
def test_pe_add_rows_is_bit_equal_per_row(cuda, rows, dtype):
    from speecht5_amd import functional as Fn
    C, wide = 128, 192
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g).to(dtype).to(cuda)
    table = torch.randn(CAP, C, generator=g).to(cuda)
    alpha = torch.tensor([0.7], device=cuda)
    for pos in _positions(rows):
        ref = {}
        for p in sorted(set(pos)):
            y = torch.full((rows, wide), CANARY, dtype=dtype, device=cuda)
            ref[p] = Fn.tts_pe_add_step(x, table, alpha, _i32([p], cuda), y)
        whole, y = _guarded((rows, wide), dtype, cuda)
        Fn.tts_pe_add_rows(x, table, alpha, _i32(pos, cuda), y)
        torch.cuda.synchronize()
        assert _guards_intact(whole, rows * wide)
        for r_, p in enumerate(pos):
            assert torch.equal(y[r_], ref[p][r_]), (r_, p)
        assert bool((y[:, C:] == CANARY).all())


# ---- step tail ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("seeds", [False, True], ids=["noseeds", "seeds"])
@pytest.mark.parametrize("rows", [3, 33])
def test_step_tail_rows_matches_the_scalar_tail_per_row(cuda, rows, seeds, dtype):
    from speecht5_amd import functional as Fn
    r, odim, thr = 2, 8, 0.5
    F = r * odim
    g = torch.Generator().manual_seed(rows)
    for si, pos in enumerate(_positions(rows)):
        y = torch.randn(rows, F + r + 3, generator=g)
        y[:, F:F + r] = torch.where(torch.rand(rows, r, generator=g) < 0.3, 2.0, -3.0)      # some rows stop on their probability
        minlen = torch.tensor([(b % 3) * 2 for b in range(rows)], dtype=torch.int32)          # 0, 2, 4: some stops are held back
        maxlen = torch.tensor([3 + b % 4 for b in range(rows)], dtype=torch.int32)           # 3 .. 6: some stops are forced
        done = torch.tensor([1 if b % 5 == 4 or (rows == 3 and si == 2 and b == 2) else 0 for b in range(rows)], dtype=torch.int32)
        steps = done * 2
        yd, mn, mx = y.to(cuda), minlen.to(cuda), maxlen.to(cuda)

        def fresh():
            mel = _guarded((rows, CAP * r, odim), torch.float32, cuda)
            prob = _guarded((rows, CAP * r), torch.float32, cuda)
            nxt = _guarded((rows, odim), dtype, cuda)
            return mel, prob, nxt, done.to(cuda), steps.to(cuda), torch.full((1,), -1, dtype=torch.int32, device=cuda)
        ref = {}
        for p in sorted(set(pos)):
            if not 0 <= p < CAP:
                continue
            mel, prob, nxt, dn, stp, act = fresh()
            Fn.tts_step_tail_dev(yd, r, odim, mn, mx, dn, stp, _i32([p], cuda), thr, mel[1], prob[1], nxt[1], act)
            ref[p] = (mel[1], prob[1], nxt[1], dn, stp)
        mel, prob, nxt, dn, stp, act = fresh()
        pos_d = _i32(pos, cuda)
        tick = table = slots = None
        if seeds:
            R_, n = 4, 2
            tick = _i32([(si + 2) % R_], cuda)
            table = torch.arange(1000, 1000 + R_ * n, dtype=torch.int64, device=cuda).view(R_, n)
            slots = torch.zeros(n, dtype=torch.int64, device=cuda)
        Fn.tts_step_tail_rows(yd, r, odim, mn, mx, dn, stp, pos_d, thr, mel[1], prob[1], nxt[1], act, tick, table, slots)
        torch.cuda.synchronize()
        for (whole, view) in (mel, prob, nxt):
            assert _guards_intact(whole, view.numel())
        running = 0
        for b, p in enumerate(pos):
            live = int(done[b]) == 0 and 0 <= p < CAP
            if not live:      # finished and out-of-range rows: untouched, not advanced
                assert bool((mel[1][b] == CANARY).all()) and bool((prob[1][b] == CANARY).all()) and bool((nxt[1][b] == CANARY).all()), b
                assert int(dn[b]) == int(done[b]) and int(stp[b]) == int(steps[b]) and int(pos_d[b]) == p, b
                continue
            m_, p_, n_, d_, s_ = ref[p]
            assert torch.equal(mel[1][b], m_[b]) and torch.equal(prob[1][b], p_[b]) and torch.equal(nxt[1][b], n_[b]), (b, p)
            assert int(dn[b]) == int(d_[b]) and int(stp[b]) == int(s_[b]) and int(pos_d[b]) == p + 1, (b, p)
            assert bool((prob[1][b, :p * r] == CANARY).all()) and bool((prob[1][b, (p + 1) * r:] == CANARY).all())
            running += int(d_[b]) == 0
        assert int(act) == running
        if seeds:
            want = (si + 3) % 4
            assert int(tick) == want and torch.equal(slots, table[want]), "the slots hold the next tick's row"


def test_step_tail_rows_tick_wraps_and_recovers(cuda):
    from speecht5_amd import functional as Fn
    r, odim, rows = 1, 4, 2
    y = torch.zeros(rows, odim + 1, device=cuda)
    z = lambda v: _i32([v] * rows, cuda)      # noqa: E731
    table = torch.arange(10, 16, dtype=torch.int64, device=cuda).view(3, 2)
    for t0, want in ((2, 0), (-5, 0), (99, 0), (0, 1)):
        tick, slots = _i32([t0], cuda), torch.zeros(2, dtype=torch.int64, device=cuda)
        Fn.tts_step_tail_rows(y, r, odim, z(0), z(9), z(1), z(0), z(0), 0.5, torch.zeros(rows, CAP, odim, device=cuda),
                              torch.zeros(rows, CAP, device=cuda), torch.zeros(rows, odim, device=cuda), _i32([0], cuda), tick, table, slots)
        assert int(tick) == want and torch.equal(slots, table[want]), t0


# ---- admission ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [3, 33])
def test_rows_admit_resets_exactly_the_admitted_rows(cuda, rows, dtype):
    from speecht5_amd import functional as Fn
    odim, D, C = 8, 16, 32
    g = torch.Generator().manual_seed(rows)
    admit = [(2, 3, 1, 4), (0, S, 0, 6)] if rows == 3 else [(32, 1, 2, 3), (0, 0, 0, 1), (17, S + 9, 5, 5), (-1, 2, 7, 7), (rows, 2, 7, 7)]
    state = {k: torch.randint(1, 50, (rows,), generator=g, dtype=torch.int32).to(cuda) for k in ("pos", "done", "steps", "minlen", "maxlen")}
    before = {k: v.clone() for k, v in state.items()}
    nxt_w, nxt = _guarded((rows, odim), dtype, cuda)
    kpm_w, kpm = _guarded((rows, S), torch.uint8, cuda, fill=7)
    cat_w, cat = _guarded((rows, C + D), dtype, cuda)
    stage = torch.randn(len(admit), D, generator=g).to(dtype).to(cuda)
    desc = torch.zeros(rows, 4, dtype=torch.int32)
    for i, a in enumerate(admit):
        desc[i] = torch.tensor(a, dtype=torch.int32)
    Fn.tts_rows_admit(desc.to(cuda), len(admit), state["pos"], state["done"], state["steps"], state["minlen"], state["maxlen"], nxt, kpm,
                      stage, cat[:, C:])
    torch.cuda.synchronize()
    assert _guards_intact(nxt_w, rows * odim) and _guards_intact(kpm_w, rows * S, fill=7) and _guards_intact(cat_w, rows * (C + D))
    admitted = {a[0]: (i, a) for i, a in enumerate(admit) if 0 <= a[0] < rows}
    for b in range(rows):
        if b in admitted:
            i, (_, T, mn, mx) = admitted[b]
            assert [int(state[k][b]) for k in ("pos", "done", "steps", "minlen", "maxlen")] == [0, 0, 0, mn, mx], b
            assert bool((nxt[b] == 0).all())
            assert kpm[b].tolist() == [int(j >= min(max(T, 0), S)) for j in range(S)], "kpm over the whole capacity"
            assert torch.equal(cat[b, C:], stage[i]) and bool((cat[b, :C] == CANARY).all())
        else:
            for k in state:
                assert int(state[k][b]) == int(before[k][b]), (b, k)
            assert bool((nxt[b] == CANARY).all()) and bool((kpm[b] == 7).all()) and bool((cat[b] == CANARY).all()), b
    # no rows admitted: nothing is launched, nothing changes
    Fn.tts_rows_admit(desc.to(cuda), 0, state["pos"], state["done"], state["steps"], state["minlen"], state["maxlen"], nxt, kpm)
