"""GPU tier: compacted multi-stream rounds (ess_amd/run_segmentation.py: MultiStreamSegmenter(compact=True)) and the kernel under
them, hip.state_carry_indexed (record moves between two batches of different sizes, steered by index words on the device).  What is
asserted throughout: a stream gets, bit for bit, the labels, colours and confidences it gets when every round runs all S streams --
whatever the size of the batch it was gathered into, eager or replayed."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded state-like tensors, models, the S = 3 schedule, the pins)
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests.test_hip_modules import relerr  # noqa: E402

DEV = M.DEV
GUARD, NAN16 = M.GUARD, M.NAN16
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


# ---------------------------------------------------------------------------------------------- 1. the indexed carry kernel
def _move_lists(n_dst, n_src, g):
    """-> [(n_tensors, dst_index, src_index, with_src)]: together a plain permutation, zero-fills, dst words -2 / -1 / n_dst, src words
    -2 / n_src, a list longer than n_dst whose extra moves are all skipped, one shorter than n_dst, and src=None with zero-fills
    and skips only.  No valid dst word appears twice in a list."""
    Z = -1
    perm = torch.randperm(n_dst, generator=g).tolist()
    sperm = torch.randperm(n_src, generator=g).tolist()
    plain = (15, perm, [sperm[p % n_src] for p in range(n_dst)], True)
    words = [Z, sperm[0], -2, n_src, sperm[-1], I32_MAX, Z, I32_MIN, sperm[n_src // 2]]
    longer = (7, perm + [-2, -1, n_dst, n_dst + 5, I32_MIN, I32_MAX],
              [words[p % len(words)] for p in range(n_dst)] + [0, Z, 0, Z, sperm[0], Z], True)
    k = max(1, n_dst // 2)  # (n_dst = 1 has no shorter list)
    shorter = (2, perm[:k], [Z if p % 2 else sperm[p % n_src] for p in range(k)], True)
    no_src = (1, perm + [n_dst, -1], [(Z, 0, -2)[p % 3] for p in range(n_dst)] + [Z, Z], False)
    return [plain, longer, shorter, no_src]


@pytest.mark.parametrize('n_dst,n_src', [(1, 1), (8, 3), (3, 8), (9, 9)])
def test_state_carry_indexed_exact(n_dst, n_src):
    """bit-exact against a restatement with torch indexing on int16 views; records no move names and the guard bytes around every
    destination keep their NaN pre-fill; 1, 2, 7 and 15 tensors"""
    from ess_amd import hip
    assert hip.CARRY_SRC_ZERO == -1
    g = torch.Generator().manual_seed(1000 * n_dst + n_src)
    dsts = M._state_like(n_dst, g)
    srcs = dsts if n_src == n_dst else M._state_like(n_src, g)
    assert min(d[0].numel() * d.element_size() for _, d, _ in dsts) == 16
    assert max(d[0].numel() * d.element_size() for _, d, _ in dsts) > 2 * 2 ** 20
    for case, (n, di, si, with_src) in enumerate(_move_lists(n_dst, n_src, g)):
        sel = slice(0, n) if case % 2 == 0 else slice(15 - n, 15)
        pick = [(buf, dst, s[2]) for (buf, dst, _), s in zip(dsts[sel], srcs[sel])]
        for buf, _, _ in pick:
            buf.fill_(NAN16)
        before = [buf.clone() for buf, _, _ in pick]
        d_idx = torch.tensor(di, dtype=torch.int32, device=DEV)
        s_idx = torch.tensor(si, dtype=torch.int32, device=DEV)
        hip.state_carry_indexed([d for _, d, _ in pick], [s for _, _, s in pick] if with_src else None, d_idx, s_idx)
        for (buf, dst, src), old in zip(pick, before):
            nb = dst[0].numel() * dst.element_size()
            lo, hi = GUARD // 2, GUARD // 2 + n_dst * nb // 2
            got = buf[lo:hi].view(n_dst, nb // 2)
            want = old[lo:hi].view(n_dst, nb // 2).clone()
            sv = src.contiguous().view(torch.int16).view(n_src, nb // 2)
            for d, s in zip(di, si):
                if not 0 <= d < n_dst:
                    continue
                if s == -1:
                    want[d] = 0
                elif 0 <= s < n_src and with_src:
                    want[d] = sv[s]
            assert torch.equal(got, want), (n_dst, n_src, case, di, si, tuple(dst.shape), dst.dtype)
            assert torch.equal(buf[:lo], old[:lo]) and torch.equal(buf[hi:], old[hi:]), (n_dst, n_src, case, 'guard bytes written', tuple(dst.shape))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. / 3. the schedules
N_WIN = M.N_WIN
#   S = 5: active counts 5, 1, 2, 3, 4, 0, 3, 2, 5, 2 (3 of 5: bucket 4 with one padded slot; 5: the ride-along round).  At window 4
#   stream 2 is restarted while active; stream 4's restart is requested there too, while it is idle, and served at window 6.
ACTIVE5 = [[bool(c) for c in row] for row in ([1, 1, 1, 1, 1], [1, 0, 0, 0, 0], [0, 1, 1, 0, 0], [1, 1, 0, 1, 0], [1, 1, 1, 1, 0],
                                              [0, 0, 0, 0, 0], [1, 0, 1, 0, 1], [0, 1, 0, 1, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 1])]
RESTART5 = {4: [2, 4]}
SCHEDULES = {3: (M.ACTIVE, M.RESTART), 5: (ACTIVE5, RESTART5)}
C, H, W, K = 5, 64, 96, 11


def test_the_schedules_cover_what_they_are_meant_to():
    assert len(ACTIVE5) == N_WIN and {sum(a) for a in ACTIVE5} == {0, 1, 2, 3, 4, 5}
    assert ACTIVE5[4][2] and not ACTIVE5[4][4] and not ACTIVE5[5][4] and ACTIVE5[6][4]


@functools.lru_cache(maxsize=None)
def _grids(S):
    """one host-built grid per (window, stream), built once and read by every path (two device builds may differ in the last bit)"""
    if S == 3:
        return M._schedule_grids(C, H, W)
    grids = torch.zeros(N_WIN, S, C, H, W)
    for w in range(N_WIN):
        for s in range(S):
            grids[w, s] = O.events_to_voxel_grid(M._events(3000, H, W, 1000 * s + w + 50), C, W, H)
    return grids.to(DEV)


def _run(seg, S):
    """the schedule of S streams; a NaN grid is fed for every idle stream"""
    active, restart = SCHEDULES[S]
    grids, out = _grids(S), []
    for w in range(N_WIN):
        if w in restart:
            seg.reset(restart[w])
        g = grids[w].clone()
        for s in range(S):
            if not active[w][s]:
                g[s] = float('nan')
        out.append(seg.update(g, active[w]))
    return out


def _weights(rtype):
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    return cfg, O.synth_state_dict(O.e2vid_param_shapes(cfg), 171), O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)


def _segmenter(rtype, S, **kw):
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    cfg, sd_e, sd_d = _weights(rtype)
    return MultiStreamSegmenter(*M._models(cfg, sd_e, sd_d, K), H, W, default_options(), S, palette=SH.palette_for(K), want_confidence=True, **kw)


def _assert_same_rows(a, b, S, what):
    active, _ = SCHEDULES[S]
    for w in range(N_WIN):
        assert a[w].valid == b[w].valid == tuple(active[w]), (what, w)
        assert tuple(a[w].labels.shape) == (S, H, W) and tuple(a[w].colour.shape) == (S, H, W, 3) and tuple(a[w].confidence.shape) == (S, H, W)
        for s in range(S):
            if active[w][s]:
                assert M._same(M._row(a[w], s), M._row(b[w], s)), f'{what}: stream {s} window {w}'


@pytest.mark.parametrize('S', [3, 5])
@pytest.mark.parametrize('rtype,mode', M.CASES)
def test_compacted_rounds_equal_ride_along_rounds(rtype, mode, S):
    """compact=True against compact=False on the same schedule and grids: every active row equal in labels, colours and confidence
    bits.  The batch size now varies from round to round, so both batch-size-dependent dispatch choices are pinned on both sides."""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        ride = _run(_segmenter(rtype, S), S)
        seg = _segmenter(rtype, S, compact=True)
        assert seg.buckets == {3: (1, 2), 5: (1, 2, 4)}[S] and seg.n_captures == 0
        comp = _run(seg, S)
        _assert_same_rows(comp, ride, S, f'{rtype} {mode} S={S}: compacted differs from ride-along')
        assert seg.n_windows == N_WIN and seg.n_captures == 0
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')


@pytest.mark.parametrize('S', [3, 5])
@pytest.mark.parametrize('rtype,mode', M.CASES)
def test_replay_equals_eager_under_compaction(rtype, mode, S):
    """graph=True against eager, both compacted, bit for bit; one capture per bucket plus the ride-along one at the most, none added
    by a second pass; warm_up() makes them all at once and changes nothing a round sees; earlier results stay intact (copy=True)"""
    from ess_amd import hip
    hip.set_compute(mode)
    try:
        eager, graph = _segmenter(rtype, S, compact=True), _segmenter(rtype, S, compact=True, graph=True)
        re_, rg = _run(eager, S), _run(graph, S)
        _assert_same_rows(rg, re_, S, f'{rtype} {mode} S={S}: replay differs from eager')
        assert len({r.labels.data_ptr() for r in rg}) == N_WIN  # (fresh results: a later replay did not overwrite an earlier one)
        n_cap = graph.n_captures
        assert 1 <= n_cap <= len(graph.buckets) + 1 and eager.n_captures == 0
        graph.reset()
        again = _run(graph, S)
        assert graph.n_captures == n_cap and graph.n_windows == 2 * N_WIN
        _assert_same_rows(again, re_, S, f'{rtype} {mode} S={S}: second pass')
        _assert_same_rows(rg, re_, S, f'{rtype} {mode} S={S}: an earlier result was overwritten')
        warm = _segmenter(rtype, S, compact=True, graph=True)
        warm.warm_up()
        assert warm.n_captures == len(warm.buckets) + 1 == n_cap and warm.n_windows == 0  # (both schedules use every bucket)
        active, _ = SCHEDULES[S]
        first = warm.update(_grids(S)[0], active[0])
        assert warm.n_captures == n_cap
        for s in range(S):
            if active[0][s]:
                assert M._same(M._row(first, s), M._row(re_[0], s)), f'{rtype} {mode} S={S}: first round after warm_up, stream {s}'
    finally:
        hip.set_compute('fp32')


def test_warm_up_leaves_state_and_pending_restarts():
    """eager and replayed: a warm_up() in the MIDDLE of a schedule -- streams carrying a state, one restart pending -- changes no
    later result"""
    from ess_amd import hip
    S = 5
    active, restart = SCHEDULES[S]
    grids = _grids(S)
    ref = _run(_segmenter('convlstm', S, compact=True), S)
    for graph in (False, True):
        seg = _segmenter('convlstm', S, compact=True, graph=graph)
        for w in range(N_WIN):
            if w in restart:
                seg.reset(restart[w])
            if w == 5:  # (stream 4's restart is pending here)
                seg.warm_up()
            r = seg.update(grids[w], active[w])
            for s in range(S):
                if active[w][s]:
                    assert M._same(M._row(r, s), M._row(ref[w], s)), (graph, w, s)
        assert seg.n_captures == (len(seg.buckets) + 1 if graph else 0)
    assert hip.compute_name() == 'fp32'


# ---------------------------------------------------------------------------------------------- 4. events -> compact grids
def test_update_from_events_under_compaction():
    """two of five streams have events: ONE voxel_grid_temporal call builds the bucket's two grids, which equal the per-stream builds
    to the last-bit tolerance two atomic builds can differ by (relerr < 1e-6)"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import events_to_voxel_grid_device
    from ess_amd.run_segmentation import MultiStreamSegmenter
    K6 = 6
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K6), 172, decoder_style=True)
    seg = MultiStreamSegmenter(*M._models(cfg, sd_e, sd_d, K6), H, W, default_options(), 5, compact=True)
    built = []
    vgt = hip.voxel_grid_temporal
    try:
        hip.voxel_grid_temporal = lambda *a, **kw: (built.append(vgt(*a, **kw)), built[-1])[1]
        evs = [M._events(5000, H, W, 1), None, M._events(3000, H, W, 2), None, None]
        r = seg.update_from_events(evs)
    finally:
        hip.voxel_grid_temporal = vgt
    assert r.valid == (True, False, True, False, False) and tuple(r.labels.shape) == (5, H, W) and r.colour is None and r.confidence is None
    assert len(built) == 1 and tuple(built[0].shape) == (2, C, H, W)  # (bucket 2: only the compact grids are built)
    assert tuple(seg.compact_input.shape) == (4, C, H, W)
    for slot, s in enumerate((0, 2)):
        own = events_to_voxel_grid_device(evs[s], C, W, H, DEV)
        assert relerr(built[0][slot], own) < 1e-6
        assert torch.equal(seg.compact_input[slot], built[0][slot])
    # one active stream of five, then three (bucket 4: the padded slot is an empty slice, an all-zero grid)
    r1 = seg.update_from_events([None, None, None, evs[0], None])
    assert r1.valid == (False, False, False, True, False)
    r3 = seg.update_from_events([evs[0], evs[2], None, None, evs[0]])
    assert r3.valid == (True, True, False, False, True) and not bool(seg.compact_input[3].any())
    r0 = seg.update_from_events([None] * 5)
    assert r0.valid == (False,) * 5 and seg.n_windows == 4
    with pytest.raises(hip.EssHipError, match='n_streams=5'):
        seg.update_from_events(evs[:2])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. full size
def test_full_size_eight_streams_compacted():
    """S = 8, 2 x 480 x 640, K = 11, 'mixed', graph replay, six windows with 8, 2, 3, 1, 5, 8 active streams, stream 3 restarted at
    window 2: every active row equals the compact=False run of the same schedule; finite, labels < K, colours = palette[labels]"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    S, C2, H2, W2, n_win = 8, 2, 480, 640, 6
    active = [[True] * 8, [s in (3, 6) for s in range(8)], [s in (0, 3, 7) for s in range(8)], [s == 5 for s in range(8)],
              [s in (1, 2, 3, 4, 6) for s in range(8)], [True] * 8]
    assert [sum(a) for a in active] == [8, 2, 3, 1, 5, 8]
    cfg = O.e2vid_config(num_bins=C2)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 31)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 32, decoder_style=True)
    pal = SH.palette_for(K)
    g = torch.Generator().manual_seed(78)
    grids = (torch.randn(n_win, S, C2, H2, W2, generator=g) * (torch.rand(n_win, S, C2, H2, W2, generator=g) < 0.2)).to(DEV)
    hip.set_compute('mixed')
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        def run(compact):
            seg = MultiStreamSegmenter(*M._models(cfg, sd_e, sd_d, K), H2, W2, default_options(), S, graph=True, palette=pal,
                                       want_confidence=True, compact=compact)
            out = []
            for w in range(n_win):
                if w == 2:
                    seg.reset([3])
                out.append(seg.update(grids[w], active[w]))
            assert seg.n_captures == (4 if compact else 1)  # (ride-along + buckets 2, 4, 1)
            return out
        ride, comp = run(False), run(True)
        pal_dev = pal.to(DEV) if torch.is_tensor(pal) else torch.as_tensor(pal).to(DEV)
        for w in range(n_win):
            assert comp[w].valid == ride[w].valid == tuple(active[w])
            rows = [s for s in range(S) if active[w][s]]
            for s in rows:
                assert M._same(M._row(comp[w], s), M._row(ride[w], s)), f'window {w}: stream {s} differs under compaction'
            lab, col, conf = comp[w].labels[rows], comp[w].colour[rows], comp[w].confidence[rows]
            assert bool(torch.isfinite(conf).all()) and int(lab.max()) < K
            assert torch.equal(col, pal_dev[lab.long()])
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')
