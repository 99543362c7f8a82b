"""GPU tier: multi-stream streaming segmentation (ess_amd/run_segmentation.py: MultiStreamSegmenter) and the two kernels under it --
hip.state_carry_masked (HOLD / TAKE / ZERO per stream, all state tensors in one launch) and hip.event_normalize_samples (per-sample
statistics, bit-identical per sample to hip.event_normalize).  What is asserted throughout: a stream's results do not depend on the
batch it rides in, on the other streams' schedules, or on eager issue versus graph replay -- bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests.test_hip_modules import relerr  # noqa: E402

DEV = torch.device('cuda:0')
GUARD = 256  # bytes in front of and behind every destination
NAN16 = 0x7FC0  # a NaN in bfloat16 and IEEE half; twice in a row a NaN in fp32


def _events(n, H, W, seed):
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.0, 0.2, n))
    return np.stack([t, g.integers(0, W, n).astype(np.float64), g.integers(0, H, n).astype(np.float64), g.integers(0, 2, n).astype(np.float64)], 1)


def _models(cfg, sd_e, sd_d, K):
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.models.style_networks import SemSegE2VID
    m = E2VIDRecurrent(dict(cfg))
    m.load_state_dict(sd_e)
    d = SemSegE2VID(256, K, skip_connect=True, skip_type='concat')
    d.load_state_dict(sd_d)
    return m.cuda().eval(), d.cuda().eval()


def _same(a, b):
    """labels, colour and confidence (as bits) of two results / result rows"""
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def _row(r, s):
    return r.labels[s], r.colour[s], r.confidence[s]


# ---------------------------------------------------------------------------------------------- 1. the carry kernel
def _guarded(shape, dtype):
    """a destination inside a NaN-filled buffer with GUARD bytes on either side -> (whole buffer as int16, the tensor)"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((n + 2 * GUARD) // 2,), NAN16, dtype=torch.int16, device=DEV)
    return buf, buf[GUARD // 2:(GUARD + n) // 2].view(dtype).view(shape)


def _state_like(S, g):
    """15 tensors in the forms a carried state takes, stream index first: fp32 NCHW h and c, BF16_C8 and F16_C8 copies (one of them
    a [hi | lo] pair: 2 CB blocks), F32_C8 -- per-stream sizes from 16 bytes to 2.5 MB"""
    shapes = [((S, 64, 60, 80), torch.float32), ((S, 8, 60, 80, 8), torch.bfloat16), ((S, 8, 60, 80, 8), torch.float16),
              ((S, 8, 60, 80, 8), torch.float32), ((S, 64, 60, 80), torch.float32),
              ((S, 128, 30, 40), torch.float32), ((S, 16, 30, 40, 8), torch.bfloat16), ((S, 2 * 32, 15, 20, 8), torch.float16),
              ((S, 256, 60, 40), torch.float32), ((S, 4), torch.float32), ((S, 1, 1, 1, 8), torch.bfloat16), ((S, 1, 1, 1, 8), torch.float16),
              ((S, 3, 8, 12), torch.float32), ((S, 2, 8, 12, 8), torch.bfloat16), ((S, 40), torch.float16)]
    out = []
    for shape, dt in shapes:
        buf, dst = _guarded(shape, dt)
        src = torch.randn(shape, generator=g, dtype=torch.float32).to(dt).to(DEV)
        out.append((buf, dst, src))
    return out


@pytest.mark.parametrize('S', [1, 3, 8, 9])
def test_state_carry_masked_exact(S):
    """bit-exact against the torch.where restatement on integer views; HOLD streams and the guard bytes around every destination keep
    their NaN pre-fill; src=None is accepted when no stream TAKEs; any number of tensors from 1 to 15"""
    from ess_amd import hip
    g = torch.Generator().manual_seed(100 + S)
    Hd, T, Z = hip.CARRY_HOLD, hip.CARRY_TAKE, hip.CARRY_ZERO
    modes = [[Hd] * S, [T] * S, [Z] * S] + [torch.randint(0, 3, (S,), generator=g).tolist() for _ in range(4)]
    tensors = _state_like(S, g)
    assert min(d[0].numel() * d.element_size() for _, d, _ in tensors) == 16
    assert max(d[0].numel() * d.element_size() for _, d, _ in tensors) > 2 * 2 ** 20
    for case, mode in enumerate(modes):
        n = (1, 2, 7, 15, 15, 15, 4)[case]
        pick = tensors[:n] if case % 2 == 0 else tensors[-n:]
        for buf, _, _ in pick:
            buf.fill_(NAN16)
        before = [buf.clone() for buf, _, _ in pick]
        m = torch.tensor(mode, dtype=torch.int32, device=DEV)
        no_take = T not in mode
        hip.state_carry_masked([d for _, d, _ in pick], None if no_take else [s for _, _, s in pick], m)
        for (buf, dst, src), old in zip(pick, before):
            nb = dst[0].numel() * dst.element_size()
            got = buf[GUARD // 2:GUARD // 2 + S * nb // 2].view(S, nb // 2)
            was = old[GUARD // 2:GUARD // 2 + S * nb // 2].view(S, nb // 2)
            sv = src.contiguous().view(torch.int16).view(S, nb // 2)
            mm = m.view(S, 1)
            want = torch.where(mm == T, sv, torch.where(mm == Z, torch.zeros_like(sv), was))
            assert torch.equal(got, want), (S, case, mode, tuple(dst.shape), dst.dtype)
            assert torch.equal(buf[:GUARD // 2], old[:GUARD // 2]) and torch.equal(buf[GUARD // 2 + S * nb // 2:], old[GUARD // 2 + S * nb // 2:]), \
                (S, case, 'guard bytes written', tuple(dst.shape))
    # a word that is none of the three is a HOLD
    buf, dst, src = tensors[0]
    buf.fill_(NAN16)
    hip.state_carry_masked([dst], [src], torch.full((S,), 7, dtype=torch.int32, device=DEV))
    assert bool((buf == NAN16).all())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. per-sample normalisation
@pytest.mark.parametrize('S', [1, 3, 8])
@pytest.mark.parametrize('chw', [(5, 64, 96), (2, 480, 640), (5, 440, 640)])
def test_event_normalize_samples_equals_the_single_tensor_kernel(S, chw):
    from ess_amd import hip
    C, H, W = chw
    g = torch.Generator().manual_seed(S * 1000 + H)
    x = torch.randn(S, C, H, W, generator=g) * (torch.rand(S, C, H, W, generator=g) < 0.3) * (1 + 3 * torch.rand(S, 1, 1, 1, generator=g))
    if S > 1:
        x[1].zero_()  # a stream without a single event: copied unchanged (the reference's num_nonzeros == 0 branch)
    x = x.to(DEV)
    ref = [hip.event_normalize(x[s:s + 1]) for s in range(S)]
    y = hip.event_normalize_samples(x)
    for s in range(S):
        assert torch.equal(y[s:s + 1].view(torch.int32), ref[s].view(torch.int32)), (S, chw, s)
    if S > 1:
        assert not bool(y[1].any())
        assert not torch.equal(ref[0], hip.event_normalize(x)[0:1])  # (the batch-global statistics are another thing)
    # HOLD: not normalised, zero-filled, the others unaffected; into a NaN-filled output, nothing left unwritten
    mode = torch.ones(S, dtype=torch.int32)
    mode[S // 2] = hip.CARRY_HOLD
    mode[S - 1] = hip.CARRY_ZERO if S > 2 else mode[S - 1]  # (any non-zero word is 'active' here)
    out = torch.full_like(x, float('nan'))
    y2 = hip.event_normalize_samples(x, mode.to(DEV), out=out)
    assert y2 is out
    for s in range(S):
        if s == S // 2:
            assert not bool(y2[s].view(torch.int32).any()), (S, chw, s)
        else:
            assert torch.equal(y2[s:s + 1].view(torch.int32), ref[s].view(torch.int32)), (S, chw, s)


# ---------------------------------------------------------------------------------------------- 3. / 5. the schedule
N_WIN = 10
#   stream 0 runs throughout; stream 1 joins at window 3 and is restarted at window 7; stream 2 is idle on windows 2 and 5
ACTIVE = [[True, w >= 3, w not in (2, 5)] for w in range(N_WIN)]
RESTART = {7: [1]}


def _schedule_grids(C, H, W, per=3000):
    """one host-built grid per (window, stream): the device's voting kernel adds with fp32 atomics, two builds may differ in the last
    bit (tests/test_hip_seg_stream.py) -- every path below reads the SAME grids"""
    grids = torch.zeros(N_WIN, 3, C, H, W)
    for w in range(N_WIN):
        for s in range(3):
            grids[w, s] = O.events_to_voxel_grid(_events(per, H, W, 1000 * s + w), C, W, H)
    return grids.to(DEV)


def _run_schedule(seg, grids):
    out = []
    for w in range(N_WIN):
        if w in RESTART:
            seg.reset(RESTART[w])
        g = grids[w].clone()
        for s in range(3):
            if not ACTIVE[w][s]:
                g[s] = float('nan')  # an idle stream's grid is not read
        out.append(seg.update(g, ACTIVE[w]))
    return out


def _pinned_s2d():
    """One form of the encoder's 5x5 / stride-2 convolutions on both sides of a batch-size comparison: which form a launch takes
    depends on the batch size (submodules._s2d_spec), the two add the same products in another order."""
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    return set_s2d_mode('2')


def _pinned_norm_split(hip):
    """... and one form of the decoder's InstanceNorm statistics: on planes too large for the single-workgroup kernels (120 x 160 and
    up) the number of slices a plane's sums are taken in follows from N * ceil(C/8) (norm_c8.hip, split_for8), i.e. from the batch size
    -- the same fp64 partial sums in another order, seen as single half-precision ulps at 480 x 640 between B = 8 and B = 1.  The
    tuning switch "norm_split_wgs" at hip.NORM_SPLIT_BY_PLANE lets the plane size alone decide.  -> the previous value"""
    prev = hip.tuning_get('norm_split_wgs')
    hip.tuning_set('norm_split_wgs', hip.NORM_SPLIT_BY_PLANE)
    return prev


CASES = [('convlstm', 'fp32'), ('convlstm', 'bf16'), ('convlstm', 'mixed'), ('convgru', 'fp32'), ('convgru', 'bf16'), ('convgru', 'mixed')]


@pytest.mark.parametrize('rtype,mode', CASES)
def test_streams_are_independent_of_their_batch(rtype, mode):
    """every stream of the S = 3 schedule gets, window by window, the labels, colours and confidences (bits) a
    MultiStreamSegmenter(n_streams=1) gives it when fed that stream's active windows and restarts alone; valid mirrors the schedule.
    The space-to-depth form is pinned on both sides (_pinned_s2d)."""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    C, H, W, K = 5, 64, 96, 11
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    pal = SH.palette_for(K)
    grids = _schedule_grids(C, H, W)
    hip.set_compute(mode)
    prev = _pinned_s2d()
    try:
        batch = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 3, palette=pal, want_confidence=True)
        res = _run_schedule(batch, grids)
        assert [r.valid for r in res] == [tuple(a) for a in ACTIVE]
        assert res[0].labels.dtype == torch.uint8 and tuple(res[0].labels.shape) == (3, H, W) and tuple(res[0].colour.shape) == (3, H, W, 3)
        solo = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 1, palette=pal, want_confidence=True)
        for s in range(3):
            solo.reset()
            for w in range(N_WIN):
                if s in RESTART.get(w, ()):
                    solo.reset([0])
                if not ACTIVE[w][s]:
                    continue
                r = solo.update(grids[w, s:s + 1])
                assert r.valid == (True,)
                assert _same(_row(res[w], s), _row(r, 0)), f'{rtype} {mode}: stream {s} window {w} depends on its batch'
    finally:
        set_s2d_mode(prev)
        hip.set_compute('fp32')


@pytest.mark.parametrize('rtype,mode', CASES)
def test_replay_equals_eager_on_the_schedule(rtype, mode):
    """graph replay == eager issue bit for bit in every window of the schedule, the first included; results handed out earlier stay
    intact (copy=True); ONE capture serves every mix of advancing, idle and restarting streams"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    C, H, W, K = 5, 64, 96, 11
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    pal = SH.palette_for(K)
    grids = _schedule_grids(C, H, W)
    hip.set_compute(mode)
    try:
        eager = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 3, palette=pal, want_confidence=True)
        graph = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 3, graph=True, palette=pal, want_confidence=True)
        re_, rg = _run_schedule(eager, grids), _run_schedule(graph, grids)
        for w in range(N_WIN):
            assert rg[w].valid == re_[w].valid == tuple(ACTIVE[w])
            for s in range(3):
                if ACTIVE[w][s]:
                    assert _same(_row(re_[w], s), _row(rg[w], s)), f'{rtype} {mode}: replay differs from eager, stream {s} window {w}'
        assert len({r.labels.data_ptr() for r in rg}) == N_WIN  # (clones: a later replay did not overwrite an earlier result)
        assert graph.n_captures == 1 and eager.n_captures == 0 and graph.n_windows == eager.n_windows == N_WIN
    finally:
        hip.set_compute('fp32')


# ---------------------------------------------------------------------------------------------- 4. against the single-stream driver
def _latent_values(hip, lat):
    """fp32 values of the latents {1, 2, 4, 8} handed to predict, whatever form the configuration leaves them in"""
    from ess_amd import copies
    out = []
    for k in (1, 2, 4, 8):
        t = lat[k]
        if not copies.of(t).unwritten:
            out.append(t.float())
            continue
        c8, h16 = copies.of(t).c8, copies.of(t).h16
        if c8 is not None:
            out.append(c8.float())
        else:
            h, hilo = h16
            h = h.float()
            out.append(h[:, :h.shape[1] // 2] + h[:, h.shape[1] // 2:] if hilo else h)
    return out


@pytest.mark.parametrize('rtype,mode', CASES)
def test_one_stream_against_streaming_segmenter(rtype, mode):
    """MultiStreamSegmenter(n_streams=1) and StreamingSegmenter on the same six windows, reset(), six more.  The multi-stream driver
    starts a sequence from a ZERO state on the with-state launches, the single-stream one from NO state on the x-only launches.
    fp32: the kernels are an FMA chain in k order and zero products leave it unchanged -- labels and colours equal, confidences
    bit-equal.  bf16 / mixed: the bound set for them is relerr < 2e-2 on the latents handed to predict (the bound
    tests/test_hip_modules.py uses for two fp32 summation orders of the same low-precision products), with label disagreements
    recorded as counts; on the MI355X the results turned out BIT-EQUAL there too (latents, labels, colours, confidences, all twelve
    windows, ConvLSTM and ConvGRU: the matrix-core kernels also add the h products behind the x products, and exact zeros change
    nothing), so equality is what is asserted in every configuration."""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter, StreamingSegmenter
    from tests.conftest import record_parity
    C, H, W, K, n_win, per = 5, 64, 96, 11, 6, 4000
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    pal = SH.palette_for(K)
    hip.set_compute(mode)
    try:
        multi = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 1, palette=pal, want_confidence=True)
        single = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), palette=pal, want_confidence=True)
        flips, worst, bit_equal = 0, 0.0, True
        for rep in range(2):
            for i in range(n_win):
                grid = O.events_to_voxel_grid(_events(per, H, W, 10 * rep + i), C, W, H).to(DEV)
                rm, rs = multi.update(grid.unsqueeze(0)), single.update(grid)
                lm, ls = _latent_values(hip, multi.last_latent), _latent_values(hip, single.last_latent)
                same = _same((rm.labels, rm.colour, rm.confidence), (rs.labels, rs.colour, rs.confidence))
                bit_equal = bit_equal and same and all(torch.equal(a, b) for a, b in zip(lm, ls))
                assert same, f'{rtype} {mode} rep {rep} window {i}: zero state and no state differ'
                err = max(relerr(a, b) for a, b in zip(lm, ls))
                worst = max(worst, err)
                flips += int((rm.labels != rs.labels).sum())
                assert err < 2e-2, (rtype, mode, rep, i, err)
                assert all(torch.equal(a, b) for a, b in zip(lm, ls)), f'{rtype} {mode} rep {rep} window {i}: latents differ'
            multi.reset()
            single.reset()
        print(f'{rtype} {mode}: MultiStreamSegmenter(1) vs StreamingSegmenter over {2 * n_win} windows: max latent relerr {worst:.3e}, '
              f'label disagreements {flips} of {2 * n_win * H * W}, bit-equal throughout: {bit_equal}')
        record_parity(f'MultiStreamSegmenter(1) vs StreamingSegmenter {rtype} {C}x{H}x{W} K={K}, {2 * n_win} windows', mode,
                      max_latent_relerr=worst, label_disagreements=flips, pixels=2 * n_win * H * W, bit_equal=bit_equal)
    finally:
        hip.set_compute('fp32')


# ---------------------------------------------------------------------------------------------- 6. events -> grids in one call
def test_update_from_events_with_an_idle_stream():
    """one voxel_grid_temporal call over the concatenated events with an EMPTY slice for the idle stream: its grid is all zero, the
    others equal the per-stream builds to the last-bit tolerance two atomic builds can differ by (relerr < 1e-6 on the grids -- not on
    the labels); the idle stream is reported invalid"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import events_to_voxel_grid_device
    from ess_amd.run_segmentation import MultiStreamSegmenter
    C, H, W, K = 5, 64, 96, 6
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    seg = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), 3)
    seen = []
    update = seg.update
    seg.update = lambda grids, active=None: (seen.append((grids.clone(), list(active))), update(grids, active))[1]
    evs = [_events(5000, H, W, 1), None, _events(3000, H, W, 2)]
    r = seg.update_from_events(evs)
    assert r.valid == (True, False, True) and tuple(r.labels.shape) == (3, H, W) and r.colour is None and r.confidence is None
    grids, active = seen[0]
    assert active == [True, False, True] and tuple(grids.shape) == (3, C, H, W)
    assert not bool(grids[1].any()), 'an empty slice must leave an all-zero grid'
    for s in (0, 2):
        own = events_to_voxel_grid_device(evs[s], C, W, H, DEV)
        assert relerr(grids[s], own) < 1e-6
    r2 = seg.update_from_events([None, None, None])
    assert r2.valid == (False, False, False) and seg.n_windows == 2
    with pytest.raises(hip.EssHipError, match='n_streams=3'):
        seg.update_from_events(evs[:2])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. full size
def test_full_size_eight_streams():
    """S = 8, 2 x 480 x 640, K = 11, 'mixed', four windows, stream 3 restarted at window 2, as a graph replay: deterministic over two
    runs; stream 3 equals an S = 1 run with the two batch-size-dependent dispatch choices pinned on both sides (the encoder's
    space-to-depth form: _pinned_s2d; the slices of the decoder's InstanceNorm statistics: _pinned_norm_split); finite, labels < K"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    S, C, H, W, K, n_win = 8, 2, 480, 640, 11, 4
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 31)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 32, decoder_style=True)
    pal = SH.palette_for(K)
    g = torch.Generator().manual_seed(77)
    grids = (torch.randn(n_win, S, C, H, W, generator=g) * (torch.rand(n_win, S, C, H, W, generator=g) < 0.2)).to(DEV)
    hip.set_compute('mixed')
    prev, prev_split = _pinned_s2d(), _pinned_norm_split(hip)
    try:
        def run(n_streams, pick):
            seg = MultiStreamSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), n_streams, graph=True, palette=pal,
                                       want_confidence=True)
            out = []
            for w in range(n_win):
                if w == 2:
                    seg.reset([3] if n_streams == S else [0])
                out.append(seg.update(grids[w][pick]))
            assert seg.n_captures == 1
            return out
        a = run(S, slice(None))
        b = run(S, slice(None))
        one = run(1, slice(3, 4))
        for w in range(n_win):
            assert _same((a[w].labels, a[w].colour, a[w].confidence), (b[w].labels, b[w].colour, b[w].confidence)), f'window {w}: not deterministic'
            assert _same(_row(a[w], 3), _row(one[w], 0)), f'window {w}: stream 3 depends on its batch'
            assert bool(torch.isfinite(a[w].confidence).all()) and int(a[w].labels.max()) < K and a[w].valid == (True,) * S
            assert torch.equal(a[w].colour.cpu(), pal[a[w].labels.cpu().long()])
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')
