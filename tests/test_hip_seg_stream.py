"""GPU tier: streaming event segmentation (ess_amd/run_segmentation.py: StreamingSegmenter) -- event windows -> label maps with the
recurrent state kept between windows, eagerly and as a hipGraph replay, against the long way round with the package's older pieces
(ImageReconstructor.update_reconstruction -> SemSegE2VID.forward -> hip.resize_nearest -> hip.argmax_confusion) and, in fp32, against
the CPU oracle.  Semantics: training/ess_trainer.py:424-493 (nearest resize of the logits, then argmax); loop:
e2vid/run_reconstruction.py:84-112.  The label rule is that of tests/test_hip_seg_head.py (fp64 scores of the class convolution on
the operands it reads, band e_top1 + e_top2, excused pixels capped at 0.1 % of a case)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import test_hip_seg_head as SH  # noqa: E402  (helpers: label rule, spy on the decoder's last activation)

DEV = torch.device('cuda:0')


def _events(n, H, W, seed):
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.0, 0.2, n))
    return np.stack([t, g.integers(0, W, n).astype(np.float64), g.integers(0, H, n).astype(np.float64), g.integers(0, 2, n).astype(np.float64)], 1)


def _models(cfg, sd_e, sd_d, K, skip=True):
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.models.style_networks import SemSegE2VID
    m = E2VIDRecurrent(dict(cfg))
    m.load_state_dict(sd_e)
    d = SemSegE2VID(256, K, skip_connect=skip, skip_type='concat' if skip else 'sum')
    d.load_state_dict(sd_d)
    return m.cuda().eval(), d.cuda().eval()


def _as_read(hip, lat):
    """the latents {2, 4, 8} in the form the decoder reads them in the active configuration (BF16_C8 tensors + their half copies in
    'mixed', fp32 otherwise), as a flat list of tensors for a bit comparison"""
    from ess_amd import functional as Fn
    out = []
    for k in (2, 4, 8):
        if Fn.c8_mode():
            c = Fn.as_c8(lat[k], want_hilo=k == 8).contiguous()
            out.append(c.view(torch.int16))
            h = hip.h16_of(c)
            if h is not None:
                out.append(h[0].view(torch.int16))
        else:
            out.append(lat[k])
    return out


def _palette(K):
    return SH.palette_for(K)


@pytest.mark.parametrize('rtype,mode', [('convlstm', 'fp32'), ('convlstm', 'bf16'), ('convlstm', 'mixed'), ('convgru', 'fp32'),
                                        ('convgru', 'bf16'), ('convgru', 'mixed')])
def test_streaming_segmenter_eager_graph_long_way_and_oracle(rtype, mode):
    """Six windows, reset(), six more.  (i) replay == eager BIT for bit in labels, colour and confidence, window by window and across
    the reset; results held from earlier windows stay intact (copy=True).  (ii) the latents the eager segmenter hands to predict are
    bit-equal to those of ImageReconstructor.update_reconstruction (full step, fp32 states) on the same grids, in the form the decoder
    reads them -- so the head is the only difference to forward -> resize_nearest -> argmax_confusion(want_pred), compared under the
    label rule.  (iii) fp32: against the CPU oracle (encoder-only steps carried over the windows -> semseg_decoder -> argmax) the way
    test_dsec_size_parity_vs_oracle holds its fp32 row: err = max |logit difference| < 1e-3, no disagreement where the oracle's top-two
    gap exceeds 2 err, at most 32 of 307200 pixels (rounded up to one pixel) disagree."""
    from ess_amd import hip
    from ess_amd.e2vid.image_reconstructor import ImageReconstructor
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import iter_windows_fixed_size
    from ess_amd.run_segmentation import StreamingSegmenter
    C, H, W, K, n_win, per = 5, 64, 96, 11, 6, 4000
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    ev = _events(n_win * per, H, W, 5)
    pal = _palette(K)
    hip.set_compute(mode)
    try:
        eager = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), graph=False, palette=pal, want_confidence=True)
        graph = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), graph=True, palette=pal, want_confidence=True)
        enc, dec = _models(cfg, sd_e, sd_d, K)
        rec = ImageReconstructor(enc, H, W, C, DEV, default_options())
        held = []
        for rep in range(2):
            rec.last_states_for_each_channel = {'grayscale': None}
            states = None
            for i, win in enumerate(iter_windows_fixed_size(ev, per)):
                # ONE grid for every path, built on the host: the device's voting kernel adds with fp32 atomics, so two builds may
                # differ in the last bit and the near-tied logits of a random-init decoder would make the oracle counts vary run to run
                grid = O.events_to_voxel_grid(win, C, W, H).cuda()
                re_ = eager.update(grid)
                lat_e = _as_read(hip, eager.last_latent)
                rg = graph.update(grid)
                assert torch.equal(re_.labels, rg.labels) and torch.equal(re_.colour, rg.colour), (rep, i)
                assert torch.equal(re_.confidence.view(torch.int32), rg.confidence.view(torch.int32)), (rep, i)
                assert re_.labels.dtype == torch.uint8 and tuple(re_.labels.shape) == (1, H, W)
                held.append((re_, rg))
                # the long way round
                _, _, lat = rec.update_reconstruction(grid.unsqueeze(0))
                lat_l = _as_read(hip, lat)
                assert len(lat_e) == len(lat_l) and all(torch.equal(a, b) for a, b in zip(lat_e, lat_l)), (rep, i, 'latents differ')
                with torch.no_grad():
                    logits, last = SH.forward_with_last(dec, lat)
                    pred = hip.argmax_confusion(hip.resize_nearest(logits, (H, W)), want_pred=True)
                z, e, _, _ = SH.head_scores(hip, dec, last, mode)
                what = f'{rtype} {mode} rep {rep} window {i}'
                SH.check_labels(re_.labels.cpu(), z, e, what + ' segmenter')
                SH.check_labels(pred.cpu(), z, e, what + ' long way')
                assert torch.equal(re_.colour.cpu(), pal[re_.labels.cpu().long()])
                ref_conf = torch.softmax(z, 1).max(1).values
                assert (re_.confidence.cpu().double() - ref_conf).abs().max().item() <= SH.CONF_TOL + 2 * e.max().item()
                if mode == 'fp32' and rep == 0:
                    with torch.no_grad():
                        _, states, olat = O.e2vid_step(sd_e, cfg, O.event_normalize(grid.cpu().unsqueeze(0)), states, encoder_only=True)
                        ologits = O.semseg_decoder(sd_d, olat)[1]
                        mine = dec(eager.last_latent)[1].cpu()
                    err = (mine - ologits).abs().max().item()
                    top2 = ologits.topk(2, dim=1).values
                    margin = top2[:, 0] - top2[:, 1]
                    mism = re_.labels.cpu().long() != ologits.argmax(1)
                    long_way = int((pred.cpu() != ologits.argmax(1)).sum())
                    print(f'{what}: max |dlogit| vs oracle {err:.2e}, disagreements {int(mism.sum())} (long way round: {long_way}), '
                          f'outside the 2 err band {int((mism & (margin > 2 * err)).sum())}')
                    assert err < 1e-3
                    assert int((mism & (margin > 2 * err)).sum()) == 0
                    assert int(mism.sum()) <= max(1, math.ceil(32 / 307200 * mism.numel()))
            assert eager.n_windows == graph.n_windows == n_win
            # results of earlier windows are intact: later replays did not overwrite what update() handed out
            assert all(torch.equal(a.labels, b.labels) and torch.equal(a.colour, b.colour) and
                       torch.equal(a.confidence.view(torch.int32), b.confidence.view(torch.int32)) for a, b in held)
            assert len({b.labels.data_ptr() for _, b in held}) == len(held)
            eager.reset()
            graph.reset()
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'mixed'])
def test_update_runs_the_encoder_only(mode):
    """a spy on the model: no residual block, E2VID decoder or prediction layer runs during update(), eager or captured"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import StreamingSegmenter
    C, H, W, K = 5, 64, 96, 6
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    hip.set_compute(mode)
    try:
        for use_graph in (False, True):
            enc, dec = _models(cfg, sd_e, sd_d, K)
            unet = enc.unetrecurrent
            ran = []
            tail = unet._tail
            unet._tail = lambda *a, **k: (ran.append('_tail'), tail(*a, **k))[1]
            spied = list(unet.resblocks) + list(unet.decoders) + [unet.pred]
            for m in spied:
                m.register_forward_hook(lambda mod, i, o: ran.append(type(mod).__name__))
                for name in ('forward', 'forward_sum', 'forward_cat', 'forward_of_sum'):
                    if hasattr(m, name):
                        fn = getattr(m, name)
                        setattr(m, name, (lambda f, n: lambda *a, **k: (ran.append(n), f(*a, **k))[1])(fn, f'{type(m).__name__}.{name}'))
            seg = StreamingSegmenter(enc, dec, H, W, default_options(), graph=use_graph)
            g = torch.Generator().manual_seed(3)
            for i in range(4):
                r = seg.update(torch.randn(C, H, W, generator=g).cuda())
                assert r.colour is None and r.confidence is None and tuple(r.labels.shape) == (1, H, W)
            assert ran == [], ran
            # the spy itself sees a full step
            enc(torch.zeros(1, C, H, W, device=DEV), None)
            assert '_tail' in ran
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'mixed'])
def test_reflection_padded_size_and_out_hw(mode):
    """60 x 90 needs reflection padding to 64 x 96 inside: the segmenter runs, returns 60 x 90 labels equal (label rule) to the long way
    round with the logits cropped to the region ImageReconstructor crops its image to; out_hw = (120, 180): equal to
    hip.resize_nearest of those cropped logits, then argmax.  Graph replay == eager here too."""
    from ess_amd import hip
    from ess_amd.e2vid.image_reconstructor import ImageReconstructor
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import StreamingSegmenter
    C, H, W, K = 5, 60, 90, 11
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    hip.set_compute(mode)
    try:
        seg = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options())
        seg_g = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), graph=True)
        big = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), out_hw=(120, 180))
        enc, dec = _models(cfg, sd_e, sd_d, K)
        rec = ImageReconstructor(enc, H, W, C, DEV, default_options())
        rec.last_states_for_each_channel = {'grayscale': None}
        cp = rec.crop
        assert not cp.is_identity and (cp.iy0, cp.ix0, cp.iy1, cp.ix1) == (2, 3, 62, 93)
        g = torch.Generator().manual_seed(9)
        for i in range(3):
            grid = (torch.randn(1, C, H, W, generator=g) * (torch.rand(1, C, H, W, generator=g) < 0.3)).cuda()
            r, rg, rb = seg.update(grid), seg_g.update(grid), big.update(grid)
            assert tuple(r.labels.shape) == (1, 60, 90) and tuple(rb.labels.shape) == (1, 120, 180)
            assert torch.equal(r.labels, rg.labels)
            _, _, lat = rec.update_reconstruction(grid)
            assert all(torch.equal(a, b) for a, b in zip(_as_read(hip, seg.last_latent), _as_read(hip, lat))), 'latents differ'
            with torch.no_grad():
                logits, last = SH.forward_with_last(dec, lat)
            assert tuple(logits.shape) == (1, K, 64, 96)
            z, e, _, _ = SH.head_scores(hip, dec, last, mode)
            crop = lambda t: t[:, :, cp.iy0:cp.iy1, cp.ix0:cp.ix1].contiguous()  # noqa: E731
            zc, ec, lc = crop(z), crop(e), crop(logits)
            SH.check_labels(r.labels.cpu(), zc, ec, f'{mode} padded window {i}')
            SH.check_labels(hip.argmax_confusion(lc, want_pred=True).cpu(), zc, ec, f'{mode} padded window {i} long way')
            # the device's own resize of a plane of pixel indices gives ITS source pixel per output pixel
            idx = torch.arange(60 * 90, dtype=torch.float32).view(1, 1, 60, 90).cuda()
            src = hip.resize_nearest(idx, (120, 180)).cpu().long().view(-1)
            zr = zc.reshape(1, K, -1)[:, :, src].view(1, K, 120, 180)
            er = ec.reshape(1, K, -1)[:, :, src].view(1, K, 120, 180)
            SH.check_labels(rb.labels.cpu(), zr, er, f'{mode} padded window {i} out_hw')
            SH.check_labels(hip.argmax_confusion(hip.resize_nearest(lc, (120, 180)), want_pred=True).cpu(), zr, er, f'{mode} padded window {i} out_hw long way')
    finally:
        hip.set_compute('fp32')


def test_from_checkpoints(tmp_path):
    """an E2VID checkpoint in the layout test_load_model_reads_the_reference_checkpoint_layout writes + a CheckpointSaver file with a
    'back_end' entry -> the same labels as the models built directly"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import StreamingSegmenter
    from ess_amd.utils.saver import CheckpointSaver
    C, H, W, K = 2, 64, 96, 6
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type='convgru')
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 5)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 6, decoder_style=True)
    torch.save({'arch': 'E2VIDRecurrent', 'state_dict': sd_e, 'config': {'model': dict(cfg)}}, tmp_path / 'e2vid.pth.tar')
    _, dec = _models(cfg, sd_e, sd_d, K)
    CheckpointSaver(str(tmp_path)).save_checkpoint({'back_end': dec.cpu()}, {}, epoch=3, step_count=1, batch_size_a=1, batch_size_b=1)
    pal = _palette(K)
    for mode in ('fp32', 'bf16'):
        hip.set_compute(mode)
        try:
            a = StreamingSegmenter.from_checkpoints(str(tmp_path / 'e2vid.pth.tar'), str(tmp_path / 'Epoch_3.pt'),
                                                    dict(num_classes=K, height=H, width=W, palette=pal.numpy()), want_confidence=True)
            b = StreamingSegmenter(*_models(cfg, sd_e, sd_d, K), H, W, default_options(), palette=pal, want_confidence=True)
            g = torch.Generator().manual_seed(1)
            for i in range(3):
                grid = torch.randn(C, H, W, generator=g).cuda()
                ra, rb = a.update(grid), b.update(grid)
                assert torch.equal(ra.labels, rb.labels) and torch.equal(ra.colour, rb.colour) and torch.equal(ra.confidence, rb.confidence)
        finally:
            hip.set_compute('fp32')
    torch.save({'optimizer_back': {}}, tmp_path / 'Epoch_4.pt')
    with pytest.raises(hip.EssHipError, match='back_end'):
        StreamingSegmenter.from_checkpoints(str(tmp_path / 'e2vid.pth.tar'), str(tmp_path / 'Epoch_4.pt'), dict(num_classes=K, height=H, width=W))
