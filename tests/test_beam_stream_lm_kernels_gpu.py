"""st5_beam_lm_logprobs_sents (csrc/beam_lm.hip) alone: the per-slot form of the LM term of a beam search step, compared BY BYTES with
the scalar kernel st5_beam_lm_logprobs at the slot's own step (the method of tests/test_beam_stream_ctc_kernels_gpu.py).  3 slots, cap
4, w = 0.3; both forms (with decoder logits at T = 1 and 0.25, and in place), fp32 and bf16 LM logits, in row buffers wider than V /
V_lm.  `lp` is poison-filled before every launch in both arms (the in-place form then gets its mixed log-probabilities in columns
0 .. V - 1), so what a kernel leaves alone compares equal too.  Every shape has -inf decoder logits, -inf LM logits and -inf mixed
log-probabilities; one decoder logit is NaN.

1. all slots at one step: steps 0 .. cap equal the scalar kernel at that counter; one past the limit not a byte is written;
2. staggered slots at pos = (0, 2, maxlen) under their own limits: each slot equals a one-sentence launch of the scalar kernel at its
   own step and limit; then one slot done and one idle (as BeamStreamState starts it): neither changes a byte of lp;
3. a maxlen above the cap is clamped to the cap;
4. w = 0 in the logits form gives st5_beam_ctc_candidates_sents' lp, bit for bit (finite LM logits here: 0 * -inf is NaN in the
   generator's torch expression too; the NaN entries of the row with the NaN logit are compared as a pattern, as
   tests/test_beam_lm_step_gpu.py compares the scalar kernel's);
5. the argument checks return ST5_ERR_ARG."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SLOTS, CAP, EOS, W = 3, 4, 2, 0.3
SHAPES = [(36, 34, 1), (83, 83, 3), (5000, 4998, 3), (1000, 1000, 10)]
FORMS = [("logits", 1.0), ("logits", 0.25), ("inplace", 1.0)]
POISON = float.fromhex("-0x1.23456p+100")
NINF = float("-inf")


def _b(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


class Arms:
    """Decoder logits, LM logits and mixed log-probabilities of one shape, shared by both arms: rows = 3 slots x beam, every row buffer
    wider than what may be read (1e9 behind V / V_lm: a read past the end would show in the statistics)."""

    def __init__(self, cuda, V, V_lm, beam, T, lm_dtype, finite_lm=False):
        g = torch.Generator().manual_seed(11 + V + beam)
        rows = self.rows = N_SLOTS * beam
        self.cuda, self.V, self.V_lm, self.beam, self.T = cuda, V, V_lm, beam, T
        logits = torch.full((rows, V + 3), 1e9)
        logits[:, :V] = torch.randn(rows, V, generator=g) * 3 * T
        logits[0, 5] = logits[rows - 1, V - 1] = logits[rows // 2, 0] = NINF
        logits[min(1, rows - 1), 9] = float("nan")
        lm = torch.full((rows, V_lm + 5), 1e9)
        lm[:, :V_lm] = torch.randn(rows, V_lm, generator=g) * 4
        if not finite_lm:
            lm[0, 7] = lm[rows - 1, V_lm - 1] = lm[rows // 2, 1] = NINF
        mixed = torch.log_softmax(torch.randn(rows, V, generator=g) * 3, -1)
        mixed[:, 1::7] = 0.6 * mixed[:, 1::7] - 0.4 * torch.rand(rows, len(range(1, V, 7)), generator=g) * 5
        mixed[0, 8] = mixed[rows - 1, 1] = mixed[rows // 2, V - 1] = NINF
        self.logits, self.lm, self.mixed = logits.to(cuda), lm.to(lm_dtype).to(cuda)[:, :V_lm], mixed.to(cuda)
        assert self.logits.stride(0) > V and self.lm.stride(0) > V_lm

    def fresh_lp(self, form, rows=None):
        lp = torch.full((self.rows, self.V + 2), POISON, device=self.cuda)
        if form == "inplace":
            lp[:, :self.V] = self.mixed
        return lp if rows is None else lp[rows[0]:rows[1]]

    def sents(self, form, pos, maxlen, done, w=W):
        """One launch of the per-slot form over all slots; returns lp."""
        from speecht5_amd import functional as Fn
        ss = Fn.BeamStreamState(N_SLOTS, self.beam, CAP, self.cuda)
        i32 = dict(dtype=torch.int32, device=self.cuda)
        ss.pos.copy_(torch.tensor(pos, **i32))
        ss.maxlen.copy_(torch.tensor(maxlen, **i32))
        ss.done.copy_(torch.tensor(done, **i32))
        lp = self.fresh_lp(form)
        Fn.beam_lm_logprobs_sents(lp, self.V, ss, self.lm, w, logits=self.logits if form == "logits" else None, temperature=self.T)
        return lp

    def scalar(self, form, slots, counter, max_len):
        """One launch of the scalar kernel over the rows of the consecutive slots `slots` at `counter` under `max_len`; returns their lp."""
        from speecht5_amd import functional as Fn
        r0, r1 = slots[0] * self.beam, (slots[-1] + 1) * self.beam
        bs = Fn.BeamStepState(len(slots), self.beam, max_len, EOS, self.cuda)
        bs.counter.fill_(counter)
        lp = self.fresh_lp(form, (r0, r1))
        Fn.beam_lm_logprobs(lp, self.V, bs, self.lm[r0:r1], W, logits=self.logits[r0:r1] if form == "logits" else None, temperature=self.T)
        return lp

    def untouched(self, form, slot):
        return self.fresh_lp(form, (slot * self.beam, (slot + 1) * self.beam))


def _rows(t, slot, beam):
    return t[slot * beam:(slot + 1) * beam]


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,T", FORMS, ids=["logits-T1", "logits-T0.25", "inplace"])
@pytest.mark.parametrize("V,V_lm,beam", SHAPES)
def test_equal_positions_are_the_scalar_kernel_at_that_counter(cuda, V, V_lm, beam, form, T, lm_dtype):
    a = Arms(cuda, V, V_lm, beam, T, lm_dtype)
    for step in range(CAP + 2):                         # steps 0 .. cap and one past it
        got = a.sents(form, [step] * 3, [CAP] * 3, [0] * 3)
        want = a.scalar(form, [0, 1, 2], step, CAP)
        torch.cuda.synchronize()
        assert _b(got) == _b(want), f"step {step}"
        if step <= CAP:
            assert _b(got) != _b(a.fresh_lp(form)), f"step {step}: nothing was written"
        else:
            assert _b(got) == _b(a.fresh_lp(form)), "one past the limit not a byte is written"


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,T", FORMS, ids=["logits-T1", "logits-T0.25", "inplace"])
@pytest.mark.parametrize("V,V_lm,beam", SHAPES)
def test_staggered_slots_equal_one_sentence_launches_and_done_or_idle_slots_are_left_alone(cuda, V, V_lm, beam, form, T, lm_dtype):
    a = Arms(cuda, V, V_lm, beam, T, lm_dtype)
    pos, maxlen = [0, 2, CAP - 1], [CAP, CAP, CAP - 1]  # slot 2 stands at its own limit, below the cap
    got = a.sents(form, pos, maxlen, [0, 0, 0])
    single = [a.scalar(form, [s], pos[s], maxlen[s]) for s in range(N_SLOTS)]
    torch.cuda.synchronize()
    for s in range(N_SLOTS):
        assert _b(_rows(got, s, beam)) == _b(single[s]), f"slot {s}"
        assert _b(single[s]) != _b(a.untouched(form, s)), f"slot {s}: the scalar arm wrote nothing"
    # slot 1 done inside its limit, slot 2 idle as BeamStreamState starts a slot (done = 1, pos = maxlen = 0)
    got = a.sents(form, [0, 2, 0], [CAP, CAP, 0], [0, 1, 1])
    torch.cuda.synchronize()
    assert _b(_rows(got, 0, beam)) == _b(single[0])
    for s in (1, 2):
        assert _b(_rows(got, s, beam)) == _b(a.untouched(form, s)), f"a done or idle slot {s} wrote lp"
    # a slot one past its own limit below the cap, and a negative position
    got = a.sents(form, [-1, 2, CAP], [CAP, CAP, CAP - 1], [0, 0, 0])
    torch.cuda.synchronize()
    assert _b(_rows(got, 1, beam)) == _b(single[1])
    for s in (0, 2):
        assert _b(_rows(got, s, beam)) == _b(a.untouched(form, s)), f"slot {s} outside its steps wrote lp"


@pytest.mark.parametrize("form,T", FORMS, ids=["logits-T1", "logits-T0.25", "inplace"])
@pytest.mark.parametrize("V,V_lm,beam", SHAPES)
def test_a_maxlen_above_the_cap_is_clamped_to_the_cap(cuda, V, V_lm, beam, form, T):
    a = Arms(cuda, V, V_lm, beam, T, torch.float32)
    got = a.sents(form, [CAP, CAP + 1, CAP + 3], [CAP + 3] * 3, [0, 0, 0])
    want = a.scalar(form, [0], CAP, CAP)
    torch.cuda.synchronize()
    assert _b(_rows(got, 0, beam)) == _b(want)
    for s in (1, 2):
        assert _b(_rows(got, s, beam)) == _b(a.untouched(form, s)), f"slot {s}: a step past the cap wrote lp"
    got = a.sents(form, [0, 0, 0], [-2, 0, CAP], [0, 0, 0])      # a negative limit is 0: step 0 still runs
    torch.cuda.synchronize()
    assert _b(got) == _b(a.scalar(form, [0, 1, 2], 0, CAP))


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [1.0, 0.25])
@pytest.mark.parametrize("V,V_lm,beam", SHAPES)
def test_weight_zero_is_the_candidates_lp_bit_for_bit(cuda, V, V_lm, beam, T, lm_dtype):
    from speecht5_amd import functional as Fn
    a = Arms(cuda, V, V_lm, beam, T, lm_dtype, finite_lm=True)
    pos, maxlen, done = [0, 2, CAP], [CAP] * 3, [0, 0, 0]
    got = a.sents("logits", pos, maxlen, done, w=0.0)
    ss = Fn.BeamStreamState(N_SLOTS, beam, CAP, cuda)
    for name, v in (("pos", pos), ("maxlen", maxlen), ("done", done)):
        getattr(ss, name).copy_(torch.tensor(v, dtype=torch.int32, device=cuda))
    ctc = Fn.BeamCtcStreamState(ss, 2, V, min(7, V - 1), 0.4, V - 1, EOS, cuda)
    ctc.lp.fill_(POISON)
    Fn.beam_ctc_candidates_sents(a.logits, V, ss, ctc, torch.zeros(V, dtype=torch.uint8, device=cuda), T)
    torch.cuda.synchronize()
    want, got = ctc.lp, got[:, :V]
    nan = torch.isnan(want)
    assert int(nan.sum()) > 0 and not bool(nan[(torch.arange(a.rows) != min(1, a.rows - 1)).to(cuda)].any())
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.contiguous().view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def test_arguments(cuda):
    from speecht5_amd import hip
    x, y, lp = (torch.zeros(6, 40, device=cuda) for _ in range(3))
    pos = torch.full((3,), CAP + 1, dtype=torch.int32, device=cuda)        # (past the steps: nothing could be written anyway)
    ml, dn = torch.full_like(pos, CAP), torch.zeros_like(pos)

    def call(V=36, V_lm=34, lm_ld=40, lp_ld=40, n_slots=3, beam=2, cap=CAP, T=1.0, logits=x, out=lp, dt=hip.F32, p=pos, m=ml, d=dn):
        return hip.lib().st5_beam_lm_logprobs_sents(hip.ptr(logits), 40, n_slots, beam, V, T, y.data_ptr(), lm_ld, V_lm, 0.3, dt, hip.ptr(p),
                                                    hip.ptr(m), hip.ptr(d), cap, hip.ptr(out), lp_ld, hip.stream())
    assert call() == 0 and call(logits=None) == 0 and call(dt=hip.BF16) == 0
    assert call(V_lm=37) == 1, "V_lm > V"
    assert call(lm_ld=33) == 1, "an LM row stride below V_lm"
    assert call(lp_ld=35) == 1, "an lp row stride below V"
    assert call(n_slots=0) == 1 and call(beam=0) == 1 and call(beam=33) == 1 and call(cap=-1) == 1
    assert call(T=0.0) == 1 and call(out=x) == 1, "the logits form: a temperature of 0, lp aliasing the logits"
    assert call(logits=None, T=0.0) == 0, "in place the temperature is not used"
    assert call(p=None) == 1 and call(m=None) == 1 and call(d=None) == 1 and call(out=None) == 1
    assert call(dt=99) == 1
    torch.cuda.synchronize()
