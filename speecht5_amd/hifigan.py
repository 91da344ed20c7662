"""HiFi-GAN generator on the gfx950 GEMM kernel, inference only.

The reference tree has no vocoder (`SpeechT5/README.md:250` links an external one); the only concrete spec is
HuggingFace `SpeechT5HifiGan` (transformers/models/speecht5/modeling_speecht5.py:2887-3066).  This module keeps
that class's parameter names (`conv_pre`, `upsampler.{i}`, `resblocks.{j}.convs1/convs2.{k}`, `conv_post`, `mean`,
`scale`) so `microsoft/speecht5_hifigan` state dicts load, and computes on channels-last activations:

* Conv1d (dilated, "same" padding)  -> implicit GEMM over a zero-padded input, K segmented per tap
  (`seg = C, seg_stride = dilation*C`), bias + LeakyReLU / residual / running-sum fused in the epilogue; the padded input is
  made together with the LeakyReLU that precedes every convolution (`st5_pad_time_act`, one vectorised pass), or written
  directly by the producing convolution's epilogue (`out_pad`);
* ConvTranspose1d(k = 2*stride, pad = stride/2) -> `stride` phase GEMMs, each reading two adjacent input rows
  ([x[t-1], x[t]] . [W[:,:,j+stride]; W[:,:,j]]) and writing every stride-th output row;
* the mean over the resblocks is folded into the next convolution's alpha (LeakyReLU is positively homogeneous).
"""
import torch
import torch.nn as nn

from . import functional as Fn
from . import hip
from . import ragged


class HifiGanResidualBlock(nn.Module):
    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5), leaky_relu_slope=0.1):
        super().__init__()
        assert abs(leaky_relu_slope - 0.1) < 1e-12
        self.dilation = dilation
        pad = lambda k, d: (k * d - d) // 2  # noqa: E731
        self.convs1 = nn.ModuleList([nn.Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=pad(kernel_size, d))
                                     for d in dilation])
        self.convs2 = nn.ModuleList([nn.Conv1d(channels, channels, kernel_size, 1, dilation=1, padding=pad(kernel_size, 1))
                                     for _ in dilation])


def _pad_act(x, pl, pr, act=hip.ACT_NONE, lay=None, rate=1):
    """[B, L, C] -> zero-padded act(x) [B, pl + L + pr, C] in one pass (every convolution of the generator reads LeakyReLU of
    its input, zero "same"-padded: the activation and the halo are made together).  lay (a ragged.PackedLayout, B = 1): the gap
    rows of the packed sequence at upsampling rate `rate` come out zero too, in the same pass."""
    if lay is not None:
        return lay.pad_act(x, rate, pl, pr, act)
    B, L, C = x.shape
    out = torch.empty(B, L + pl + pr, C, dtype=x.dtype, device=x.device)
    hip.check(hip.lib().st5_pad_time_act(x.data_ptr(), out.data_ptr(), B, L, C, pl, pr, act, hip.dt(x), hip.stream()), "st5_pad_time_act")
    return out


def _conv_w(conv, dtype):
    """[Cout, Cin, k] -> [Cout, k*Cin] in the compute dtype (cached)."""
    return Fn._conv_w_fwd(conv.weight, dtype)


def conv_pad(conv):
    k, d = conv.weight.shape[2], conv.dilation[0]
    return (k * d - d) // 2


def conv1d(xp, L, conv, *, alpha=1.0, act=hip.ACT_NONE, residual=None, out=None, beta=0.0, out_pad=0, lay=None, rate=1):
    """Channels-last dilated 'same' Conv1d as an implicit GEMM (K segmented per tap: seg = Cin, seg_stride = dilation * Cin) over
    the PADDED input xp [B, L + 2 * conv_pad(conv), Cin]:  y = act(alpha * conv(x) + bias) + residual + beta * out.
    out_pad > 0: y is written into the interior of a fresh [B, L + 2 * out_pad, Cout] buffer with zeroed halo rows -- the layout
    the next convolution reads, no copy in between -- and that buffer is returned.  lay (a ragged.PackedLayout) with out_pad: the
    gap rows of that buffer are zeroed after the convolution wrote them (bias and activation make them non-zero)."""
    y = _conv1d(xp, L, conv, alpha, act, residual, out, beta, out_pad)
    if lay is not None and out_pad:
        lay.zero_gaps(y, rate, conv.weight.shape[0], row0=out_pad)
    return y


def _conv1d(xp, L, conv, alpha, act, residual, out, beta, out_pad):
    B, Lp, Cin = xp.shape
    Cout, _, k = conv.weight.shape
    d = conv.dilation[0]
    p = conv_pad(conv)
    assert Lp == L + 2 * p
    if out_pad:
        assert out is None and residual is None
        y = torch.empty(B, L + 2 * out_pad, Cout, dtype=xp.dtype, device=xp.device)
        hip.check(hip.lib().st5_zero_halo(y.data_ptr(), B, L, Cout, out_pad, out_pad, hip.dt(y), hip.stream()), "st5_zero_halo")
        c_op = hip.operand(y, Cout, off=out_pad * Cout, rpb=L, bstride=(L + 2 * out_pad) * Cout)
    else:
        y = out if out is not None else torch.empty(B, L, Cout, dtype=xp.dtype, device=xp.device)
        c_op = hip.operand(y, Cout)
    if xp.dtype == torch.bfloat16 and Cout in (32, 64) and Cin in (32, 64, 128):
        # few output channels: the MFMA rows are the output channels (csrc/conv1d_narrow.hip), not a 128-wide GEMM tile
        esz = 2
        hip.check(hip.lib().st5_conv1d_narrow(
            xp.data_ptr(), Lp * Cin, Cin, _conv_w(conv, xp.dtype).data_ptr(), conv.bias.detach().data_ptr(),
            y.data_ptr() + out_pad * Cout * esz, (L + 2 * out_pad) * Cout, Cout,
            hip.ptr(residual), L * Cout, Cout, B, L, Cin, Cout, k, d * Cin, alpha, beta, act, hip.stream()), "st5_conv1d_narrow")
        return y
    if xp.dtype == torch.bfloat16 and Cout == 1 and Cin % 8 == 0 and residual is None and out is None and not out_pad:
        hip.check(hip.lib().st5_conv1d_cout1(xp.data_ptr(), Lp * Cin, Cin, _conv_w(conv, xp.dtype).data_ptr(), conv.bias.detach().data_ptr(),
                                             y.data_ptr(), B, L, Cin, k, d * Cin, alpha, act, hip.stream()), "st5_conv1d_cout1")
        return y
    hip.gemm(hip.operand(xp, Cin, rpb=L, bstride=Lp * Cin, seg=Cin, seg_stride=d * Cin),
             hip.operand(_conv_w(conv, xp.dtype), k * Cin), c_op, B * L, Cout, k * Cin, hip.dt(xp),
             R=hip.operand(residual, Cout) if residual is not None else None, bias=conv.bias.detach(), act=act,
             alpha=alpha, beta=beta)
    return y


def conv_transpose1d(xp, L, convt, *, alpha=1.0):
    """Channels-last ConvTranspose1d with kernel = 2*stride, padding = stride/2 (HiFi-GAN upsampler) over the input padded by one
    row on each side, xp [B, L + 2, Cin] -> [B, s*L, Cout]."""
    B, Lp, Cin = xp.shape
    _, Cout, k = convt.weight.shape
    s = convt.stride[0]
    assert k == 2 * s and convt.padding[0] == s // 2 and Lp == L + 2
    assert s % 2 == 0, "odd stride: the transposed convolution is L * s - 1 rows long, not the L * s rows written here"
    y = torch.empty(B, L * s, Cout, dtype=xp.dtype, device=xp.device)

    def build():
        w = convt.weight.detach()  # [Cin, Cout, k]
        mats = []
        for r in range(s):
            j1 = (r + s // 2) % s
            # y[s*t' + r] = x[t1] W[:,:,j1] + x[t1-1] W[:,:,j1+s]; rows are [x[t1-1] ; x[t1]]
            mats.append(torch.cat([w[:, :, j1 + s], w[:, :, j1]], 0).t().contiguous())  # [Cout, 2*Cin]
        src = torch.stack(mats, 0)
        outw = torch.empty(src.shape, dtype=xp.dtype, device=xp.device)
        Fn._cast_into(src.view(-1, 2 * Cin), outw.view(-1, 2 * Cin))
        return outw
    Wp = Fn.weight_cache.get(("convT", xp.dtype, id(convt.weight)), [convt.weight], build)
    narrow = xp.dtype == torch.bfloat16 and Cout in (32, 64) and Cin in (32, 64, 128)
    for r in range(s):
        t_off = 0 if r < s - s // 2 else 1  # t1 = t' + t_off ; padded row index of x[t1-1] is t1
        if narrow:      # one phase = a 2-tap convolution over adjacent input rows, written to every s-th output row
            hip.check(hip.lib().st5_conv1d_narrow(
                xp.data_ptr() + t_off * Cin * 2, (L + 2) * Cin, Cin, Wp[r].data_ptr(), convt.bias.detach().data_ptr(),
                y.data_ptr() + r * Cout * 2, L * s * Cout, s * Cout, None, 0, 0, B, L, Cin, Cout, 2, Cin, alpha, 0.0, hip.ACT_NONE,
                hip.stream()), "st5_conv1d_narrow")
            continue
        hip.gemm(hip.operand(xp, Cin, off=t_off * Cin, rpb=L, bstride=(L + 2) * Cin), hip.operand(Wp[r], 2 * Cin),
                 hip.operand(y, s * Cout, off=r * Cout, rpb=L, bstride=L * s * Cout), B * L, Cout, 2 * Cin, hip.dt(xp),
                 bias=convt.bias.detach(), alpha=alpha)
    return y


class SpeechT5HifiGan(nn.Module):
    def __init__(self, model_in_dim=80, upsample_initial_channel=512, upsample_rates=(4, 4, 4, 4), upsample_kernel_sizes=(8, 8, 8, 8),
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), leaky_relu_slope=0.1,
                 normalize_before=True):
        super().__init__()
        self.num_kernels = len(resblock_kernel_sizes)
        self.num_upsamples = len(upsample_rates)
        self.normalize_before = normalize_before
        self.conv_pre = nn.Conv1d(model_in_dim, upsample_initial_channel, kernel_size=7, stride=1, padding=3)
        self.upsampler = nn.ModuleList()
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            self.upsampler.append(nn.ConvTranspose1d(upsample_initial_channel // (2 ** i), upsample_initial_channel // (2 ** (i + 1)),
                                                     kernel_size=k, stride=u, padding=(k - u) // 2))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.upsampler)):
            channels = upsample_initial_channel // (2 ** (i + 1))
            for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(HifiGanResidualBlock(channels, k, d, leaky_relu_slope))
        self.conv_post = nn.Conv1d(channels, 1, kernel_size=7, stride=1, padding=3)
        self.register_buffer("mean", torch.zeros(model_in_dim))
        self.register_buffer("scale", torch.ones(model_in_dim))

    @torch.no_grad()
    def forward(self, spectrogram):
        """[B, L, 80] (or [L, 80]) log-mel -> waveform [B, prod(rates)*L] (or 1-D), fp32."""
        is_batched = spectrogram.dim() == 3
        x = spectrogram if is_batched else spectrogram.unsqueeze(0)
        x = Fn.to_compute(x.float().contiguous())
        wav = Fn.to_float(self._generate(x)).view(x.shape[0], -1)
        return wav if is_batched else wav.view(-1)

    def _generate(self, x, lay=None):
        """The layer walk: x [B, L, model_in_dim] (compute dtype) -> [B, prod(rates) * L, 1].  lay = None: B independent rows of
        equal length.  lay = a ragged.PackedLayout (B = 1, L = lay.T): one packed sequence; the same launches, with the pad +
        activation pass selecting the gap rows to zero and the out_pad hand-over followed by a gap-zeroing pass."""
        B, L, C = x.shape
        if self.normalize_before:
            a = (1.0 / self.scale).float().contiguous()
            b = (-self.mean / self.scale).float().contiguous()
            y = torch.empty_like(x)
            hip.check(hip.lib().st5_channel_affine(x.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), B * L, C, hip.ACT_NONE,
                                                   hip.dt(x), hip.stream()), "st5_channel_affine")
            x = y
        rate = 1
        h = conv1d(_pad_act(x, 3, 3, lay=lay, rate=rate), L, self.conv_pre)
        alpha = 1.0
        LR = hip.ACT_LRELU_01
        for i in range(self.num_upsamples):
            h = conv_transpose1d(_pad_act(h, 1, 1, LR, lay=lay, rate=rate), L, self.upsampler[i], alpha=alpha)
            L = h.shape[1]
            rate *= self.upsampler[i].stride[0]
            acc = None
            for j in range(self.num_kernels):
                blk = self.resblocks[i * self.num_kernels + j]
                r = h
                n = len(blk.convs1)
                for q, (c1, c2) in enumerate(zip(blk.convs1, blk.convs2)):
                    # r -> [LeakyReLU + halo, one pass] -> c1 (+ LeakyReLU in its epilogue, written straight into c2's padded
                    # input) -> c2 (+ r in its epilogue): 7 passes over the activation per pair (round 2: 11)
                    t = conv1d(_pad_act(r, conv_pad(c1), conv_pad(c1), LR, lay=lay, rate=rate), L, c1, act=LR, out_pad=conv_pad(c2),
                               lay=lay, rate=rate)
                    if q == n - 1:   # last pair: accumulate the block output into the running sum of the resblocks
                        if acc is None:
                            acc = conv1d(t, L, c2, residual=r)
                        else:
                            conv1d(t, L, c2, residual=r, out=acc, beta=1.0)
                    else:
                        r = conv1d(t, L, c2, residual=r)
            h = acc
            alpha = 1.0 / self.num_kernels  # mean over resblocks, applied by the next convolution
        return conv1d(_pad_act(h, 3, 3, hip.ACT_LRELU_001, lay=lay, rate=rate), L, self.conv_post, alpha=alpha, act=hip.ACT_TANH)  # [B, L_out, 1]

    # ---- ragged batches: B rows of different lengths in one packed sequence (speecht5_amd/ragged.py) ----
    # Default chunk cap.  The largest stage holds E = max over the stages of (rate * channels) elements per mel frame (the last
    # one at full size: 256 * 32 = 8192).  Inside a resblock pair six buffers of that stage are alive at once: the upsampler output
    # h (the first pair's residual), the running sum acc, the residual r, its padded LeakyReLU, the hand-over buffer t and the
    # pair's output.  RAGGED_BYTE_BUDGET bounds those six:  max_frames = budget / (6 * E * element size), 5461 mel frames in
    # fp32 and 10922 in bf16 at full size (63 s / 127 s of audio at 16 kHz, hop 256).
    RAGGED_BYTE_BUDGET = 1 << 30
    RAGGED_LIVE_BUFFERS = 6

    def _ragged_meta(self):
        """(gap, elements per mel frame of the widest stage, prod(rates)), read from the module once: kernel sizes, dilations,
        strides and channel counts are fixed at construction."""
        meta = self.__dict__.get("_ragged_meta_cache")
        if meta is None:
            rate, elems = 1, self.conv_pre.weight.shape[0]
            for up in self.upsampler:
                rate *= up.stride[0]
                elems = max(elems, rate * up.weight.shape[1])
            meta = self.__dict__["_ragged_meta_cache"] = (ragged.hifigan_gap(self), elems, rate)
        return meta

    def frame_elems(self):
        """Elements per mel frame of the widest stage."""
        return self._ragged_meta()[1]

    def default_max_frames(self, dtype=None):
        esz = 2 if (dtype or Fn.compute_dtype()) == torch.bfloat16 else 4
        return max(1, self.RAGGED_BYTE_BUDGET // (self.RAGGED_LIVE_BUFFERS * self.frame_elems() * esz))

    def frame_limit(self):
        """Hard limit of one packed sequence: every buffer of it stays below 2^31 BYTES in fp32 (halo rows included), so the 32-bit
        row and element counts of the kernels on the path (st5_gemm with rpb, st5_conv1d_narrow, st5_conv1d_cout1,
        st5_batchnorm_act_fwd) hold whatever their offset types are."""
        return ((1 << 31) - 1) // (4 * self.frame_elems()) - 64

    def ragged_gap(self):
        """G of the gap rule (speecht5_amd/ragged.py) for this generator: 7 at full size."""
        return self._ragged_meta()[0]

    def _packed_rate(self):
        return self._ragged_meta()[2]

    def forward_packed(self, x, lay):
        """x [lay.T, model_in_dim] in the compute dtype (gap rows may hold anything) -> packed waveform [lay.T * prod(rates)] in the
        compute dtype (gap rows hold anything).  lay.gap must be at least ragged_gap()."""
        assert lay.gap >= self.ragged_gap(), (lay.gap, self.ragged_gap())
        if lay.T > self.frame_limit():
            raise ValueError(f"a packed sequence of {lay.T} mel frames exceeds the limit of {self.frame_limit()}")
        return self._generate(x.view(1, lay.T, -1), lay).view(-1)

    @torch.no_grad()
    def forward_ragged(self, mels, max_frames=None, lengths=None):
        """B log-mel rows of different lengths -> B one-dimensional fp32 waveforms of prod(rates) * L_b samples, each equal to
        forward(mel_b) of that row alone.  `mels`: a list of [L_b, 80] tensors, or a padded [B, L_max, 80] tensor with `lengths`;
        L_b >= 1.  Rows are packed in order into chunks of at most `max_frames` mel frames, gaps included (default: see
        RAGGED_BYTE_BUDGET); a longer row gets a chunk of its own, and a chunk of one row is the single-row call."""
        rows_in = ragged.Rows(mels, lengths)
        lengths = rows_in.lengths
        gap = self.ragged_gap()
        if max_frames is None:
            max_frames = self.default_max_frames()
        max_frames = min(int(max_frames), self.frame_limit())
        S = self._packed_rate()
        out = [None] * len(lengths)
        for rows in ragged.plan_chunks(lengths, gap, max_frames):
            if len(rows) == 1:       # a row alone in its chunk has no neighbour to be kept apart from: the single-row call itself
                out[rows[0]] = self.forward(rows_in.row(rows[0]))
                continue
            src, Lmax = rows_in.source()
            lay = ragged.PackedLayout([lengths[b] for b in rows], gap, [b * Lmax for b in rows], src.device)
            w = self.forward_packed(lay.pack_rows(src, Fn.compute_dtype()), lay)
            _, per_row = lay.unpack_rows(w, S)
            for b, wav in zip(rows, per_row):
                out[b] = wav.reshape(-1)
        return out
