"""Packed ("ragged") batches of the text-to-waveform path: layout, gap rule, chunk planner and the csrc/ragged.hip wrappers.

B utterances of L_b mel frames are packed along time into ONE sequence, each followed by a gap of G zero mel frames; row b sits
at mel offset o_b, and at a stage whose cumulative upsampling rate is s it occupies rows [s * o_b, s * (o_b + L_b)).  The rule
that makes every row equal to its single-row result: every buffer a convolution reads has zeros in its gap rows.  Then each
convolution sees around each utterance exactly the zero "same" padding of a single-row call, provided the gap is as wide as the
widest halo:  G = max over the convolutions of ceil(pad / rate at that convolution's input)  (`halo_gap`).  One gap is the right
halo of one row and the left halo of the next.  The wasted work is G / mean(L_b); a padded [B, L_max] batch with the same zeroing
would waste the spread of the lengths instead.

The layout functions are host-only (no GPU, no library): tests/test_tts_wave_cpu.py checks them without a device."""
import numpy as np
import torch

from . import hip


def halo_gap(convs):
    """convs: iterable of (pad, rate): a convolution with `pad` halo rows per side reading a buffer at cumulative upsampling
    rate `rate`.  The gap in mel frames that covers every halo."""
    return max(-(-int(p) // int(r)) for p, r in convs)


def hifigan_convs(vocoder):
    """(pad, rate) of every convolution of a SpeechT5HifiGan, read from the module."""
    out = [(vocoder.conv_pre.padding[0], 1)]
    rate = 1
    nk = vocoder.num_kernels
    for i, up in enumerate(vocoder.upsampler):
        out.append((1, rate))    # ConvTranspose1d(k = 2 * stride, padding = stride / 2): an output row reads x[t - 1], x[t] or x[t], x[t + 1]
        rate *= up.stride[0]
        for blk in vocoder.resblocks[i * nk:(i + 1) * nk]:
            out += [(c.padding[0], rate) for c in list(blk.convs1) + list(blk.convs2)]
    out.append((vocoder.conv_post.padding[0], rate))
    return out


def hifigan_gap(vocoder):
    return halo_gap(hifigan_convs(vocoder))


def postnet_gap(postnet):
    """`postnet`: modules.speech_decoder_postnet.Postnet (blocks of Conv1d + BatchNorm1d at mel rate)."""
    return halo_gap((blk[0].padding[0], 1) for blk in postnet.postnet)


def plan_chunks(lengths, gap, max_frames):
    """Rows in order into chunks of at most `max_frames` mel frames, gaps included (a row costs L_b + gap).  A row longer than the
    cap gets a chunk of its own.  Returns a list of lists of row indices; every row is in exactly one chunk."""
    chunks, cur, used = [], [], 0
    for b, n in enumerate(lengths):
        n = int(n)
        if n < 1:
            raise ValueError(f"row {b} has {n} frames; every row needs at least one")
        cost = n + gap
        if cur and max_frames is not None and used + cost > max_frames:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(b)
        used += cost
    if cur:
        chunks.append(cur)
    return chunks


def layout_tables(lengths, gap, src_starts):
    """Host tables of one packed sequence (numpy int32): `offsets` o_b, total frames T = sum(L_b + gap), `pack` [T] = the source
    row of every packed frame (src_starts[b] + t - o_b inside row b, -1 in a gap), `unpack` [sum L_b] = the packed frame of every
    valid frame in row order, `gaps` = the gap frames."""
    lengths = [int(n) for n in lengths]
    offsets, o = [], 0
    for n in lengths:
        offsets.append(o)
        o += n + gap
    T = o
    pack = np.full(T, -1, dtype=np.int32)
    for ob, n, s0 in zip(offsets, lengths, src_starts):
        pack[ob:ob + n] = np.arange(int(s0), int(s0) + n, dtype=np.int32)
    unpack = np.nonzero(pack >= 0)[0].astype(np.int32)
    gaps = np.nonzero(pack < 0)[0].astype(np.int32)
    return offsets, T, pack, unpack, gaps


class PackedLayout:
    """One packed sequence on the device.  The tables are built once per call and sent in one copy; every layer reuses them."""

    def __init__(self, lengths, gap, src_starts, device):
        self.lengths = [int(n) for n in lengths]
        self.gap = int(gap)
        self.offsets, self.T, pack, unpack, gaps = layout_tables(self.lengths, gap, src_starts)
        self.n_valid, self.n_gap = len(unpack), len(gaps)
        tab = torch.from_numpy(np.concatenate([pack, unpack, gaps])).to(device, non_blocking=True)
        self.pack = tab[:self.T]
        self.unpack = tab[self.T:self.T + self.n_valid]
        self.gaps = tab[self.T + self.n_valid:]
        self.valid = (self.pack >= 0).to(torch.uint8)

    # ---- kernels ----
    def pack_rows(self, src2d, dtype):
        """src2d fp32 [rows, w] -> packed [T, w] in `dtype`, gap frames zero."""
        src2d = src2d.contiguous()
        assert src2d.dtype == torch.float32 and src2d.dim() == 2
        w = src2d.shape[1]
        out = torch.empty(self.T, w, dtype=dtype, device=src2d.device)
        hip.check(hip.lib().st5_ragged_gather_rows(src2d.data_ptr(), self.pack.data_ptr(), out.data_ptr(), self.T, src2d.shape[0], w, 0,
                                                   hip.dt(dtype), hip.stream()), "st5_ragged_gather_rows")
        return out

    def unpack_rows(self, packed, w):
        """packed [T * s, C] (fp32 or the compute dtype) with w = s * C elements per mel frame -> fp32 [sum L_b, w], the valid frames in row
        order, and its per-row views."""
        assert packed.is_contiguous() and packed.numel() == self.T * w
        out = torch.empty(self.n_valid, w, dtype=torch.float32, device=packed.device)
        hip.check(hip.lib().st5_ragged_gather_rows(packed.data_ptr(), self.unpack.data_ptr(), out.data_ptr(), self.n_valid, self.T, w, 1,
                                                   hip.dt(packed), hip.stream()), "st5_ragged_gather_rows")
        return out, list(out.split(self.lengths, 0))

    def pad_act(self, x, rate, pl, pr, act=hip.ACT_NONE):
        """x [1, T * rate, C] -> [1, pl + T * rate + pr, C] = act(x) in the valid rows, zero in the gap rows and the halo."""
        _, L, C = x.shape
        assert L == self.T * rate and x.is_contiguous()
        out = torch.empty(1, L + pl + pr, C, dtype=x.dtype, device=x.device)
        hip.check(hip.lib().st5_ragged_pad_act(x.data_ptr(), out.data_ptr(), self.valid.data_ptr(), self.T, rate, C, pl, pr, act, hip.dt(x),
                                               hip.stream()), "st5_ragged_pad_act")
        return out

    def zero_gaps(self, buf, rate, C, row0=0):
        """Zero the gap rows of `buf`, whose row `row0` is the first row of mel frame 0 (a buffer with halo rows in front)."""
        assert buf.is_contiguous() and buf.numel() >= (row0 + self.T * rate) * C
        hip.check(hip.lib().st5_ragged_zero_gaps(buf.data_ptr() + row0 * C * buf.element_size(), self.valid.data_ptr(), self.gaps.data_ptr(),
                                                 self.n_gap, self.T, rate, C, hip.dt(buf), hip.stream()), "st5_ragged_zero_gaps")
        return buf


class Rows:
    """The two input forms of the ragged entry points -- a list of [L_b, C] tensors, or a padded [B, L_max, C] tensor with its
    lengths -- as row lengths, single rows, and (built only when a chunk packs several rows) one fp32 [B * L_max, C] source."""

    def __init__(self, mels, lengths=None):
        self.mels = mels
        if isinstance(mels, (list, tuple)):
            self.lengths = [int(m.shape[0]) for m in mels]
        else:
            assert mels.dim() == 3 and lengths is not None, "a padded [B, L_max, C] batch needs its lengths"
            self.lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            assert len(self.lengths) == mels.shape[0] and max(self.lengths) <= mels.shape[1]
        self._src = None

    def row(self, b):
        return self.mels[b] if isinstance(self.mels, (list, tuple)) else self.mels[b, :self.lengths[b]]

    def source(self):
        """(fp32 [B * L_max, C], L_max): row b starts at source row b * L_max."""
        if self._src is None:
            if isinstance(self.mels, (list, tuple)):
                x = self.mels[0].new_zeros(len(self.mels), max(self.lengths), self.mels[0].shape[1], dtype=torch.float32)
                for b, m in enumerate(self.mels):
                    x[b, :self.lengths[b]] = m
            else:
                x = self.mels.float()
            self._src = (x.reshape(-1, x.shape[-1]).contiguous(), x.shape[1])
        return self._src
