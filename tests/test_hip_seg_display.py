"""GPU tier of the streaming segmenter's display: StreamingSegmenter(reconstruct=True, postprocess=True, overlay=alpha) -- the full
recurrent step on the encoder pass the segmenter runs anyway, the displayable frame and the label overlay inside the captured window --
against the plain StreamingSegmenter (labels, colours, confidence: bit for bit), StreamingReconstructor(postprocess=True) (image and
frame: bit for bit, auto-HDR on and off) and tests/viz_ref.py (the overlay: bit for bit), eagerly and as a hipGraph replay, over a
reset().  The models are the smallest pair the streaming tests build (tests/test_hip_seg_stream.py's builders)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import test_hip_seg_stream as SS  # noqa: E402  (builders: _models, _palette)
from tests import viz_ref as V  # noqa: E402

ALPHA = 0.6


def _options(**kw):
    from ess_amd.e2vid.options.inference_options import default_options
    o = default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.view(torch.int32),
                                                                       b.view(torch.uint8) if b.dtype == torch.uint8 else b.view(torch.int32))


@pytest.mark.parametrize('H,W,mode,auto_hdr', [(64, 96, 'bf16', True), (40, 52, 'bf16', False), (40, 52, 'mixed', True), (64, 96, 'fp32', False)])
def test_display_outputs_against_the_two_drivers_and_the_restatement(H, W, mode, auto_hdr):
    """Four windows, reset(), the four again -- 64 x 96 (a multiple of 8) and 40 x 52 (reflection padding to 40 x 56 inside).  Per window,
    eager and replayed: labels / colour / confidence == the plain segmenter's; image and frame == StreamingReconstructor(postprocess=True)'s;
    overlay == viz_ref.overlay(labels, frame); replay == eager; the second pass repeats the first."""
    from ess_amd import hip
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor
    from ess_amd.run_segmentation import StreamingSegmenter
    C, K, n_win = 5, 11, 4
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    pal = SS._palette(K)
    opts = _options(auto_hdr=auto_hdr, auto_hdr_median_filter_size=2)
    g = torch.Generator().manual_seed(H)
    grids = [(torch.randn(1, C, H, W, generator=g) * (torch.rand(1, C, H, W, generator=g) < 0.3)).cuda() for _ in range(n_win)]
    hip.set_compute(mode)
    try:
        kw = dict(palette=pal, want_confidence=True)
        plain = StreamingSegmenter(*SS._models(cfg, sd_e, sd_d, K), H, W, opts, **kw)
        recon = StreamingReconstructor(SS._models(cfg, sd_e, sd_d, K)[0], H, W, opts, postprocess=True)
        disp = {use_graph: StreamingSegmenter(*SS._models(cfg, sd_e, sd_d, K), H, W, opts, graph=use_graph, reconstruct=True, postprocess=True,
                                              overlay=ALPHA, **kw) for use_graph in (False, True)}
        image_only = StreamingSegmenter(*SS._models(cfg, sd_e, sd_d, K), H, W, opts, reconstruct=True, **kw)
        first_pass = []
        for rep in range(2):
            for i, grid in enumerate(grids):
                rp = plain.update(grid)
                img, _, frame = recon.update(grid)
                assert rp.image is None and rp.frame is None and rp.overlay is None
                results = {k: d.update(grid) for k, d in disp.items()}
                for use_graph, r in results.items():
                    what = (mode, rep, i, 'graph' if use_graph else 'eager')
                    assert _same(r.labels, rp.labels) and _same(r.colour, rp.colour) and _same(r.confidence, rp.confidence), what
                    assert _same(r.image, img), what
                    assert r.frame.dtype == torch.uint8 and tuple(r.frame.shape) == (1, H, W) and _same(r.frame[0], frame), what
                    want = V.overlay(r.labels.cpu().numpy(), r.frame.cpu().numpy(), pal.numpy(), ALPHA)
                    assert tuple(r.overlay.shape) == (1, H, W, 3) and np.array_equal(r.overlay.cpu().numpy(), want), what
                e, gr = results[False], results[True]
                assert all(_same(getattr(e, f), getattr(gr, f)) for f in ('labels', 'colour', 'confidence', 'image', 'frame', 'overlay'))
                assert len(np.unique(e.frame.cpu().numpy())) > 1  # (a frame, not a constant)
                if rep == 0:
                    ro = image_only.update(grid)
                    assert ro.frame is None and ro.overlay is None and _same(ro.image, img) and _same(ro.labels, rp.labels)
                    first_pass.append((e.clone(), gr))  # (copy=True: the replay's results stay intact across windows)
                else:
                    a, b = first_pass[i]
                    for f in ('labels', 'frame', 'overlay', 'image'):
                        assert _same(getattr(a, f), getattr(e, f)) and _same(getattr(b, f), getattr(gr, f)), (mode, i, f, 'second pass')
            for d in (plain, recon, *disp.values()):
                d.reset()
    finally:
        hip.set_compute('fp32')


def test_display_keywords_are_refused_where_they_do_not_fit():
    from ess_amd import hip
    from ess_amd.run_segmentation import SegmentationResult, StreamingSegmenter
    C, K, H, W = 5, 6, 64, 96
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)
    pal = SS._palette(K)

    def make(**kw):
        return StreamingSegmenter(*SS._models(cfg, sd_e, sd_d, K), H, W, _options(), **kw)
    with pytest.raises(hip.EssHipError, match='needs reconstruct'):
        make(postprocess=True)
    with pytest.raises(hip.EssHipError, match='palette'):
        make(reconstruct=True, postprocess=True, overlay=0.5)
    with pytest.raises(hip.EssHipError, match='postprocess'):
        make(reconstruct=True, overlay=0.5, palette=pal)
    with pytest.raises(hip.EssHipError, match='outside'):
        make(reconstruct=True, postprocess=True, overlay=1.5, palette=pal)
    with pytest.raises(hip.EssHipError, match="frame's size"):
        make(reconstruct=True, postprocess=True, overlay=0.5, palette=pal, out_hw=(128, 192))
    r = SegmentationResult(torch.zeros(1, 2, 2, dtype=torch.uint8))
    assert r.image is None and r.frame is None and r.overlay is None
    c = SegmentationResult(*(torch.zeros(1) for _ in range(6))).clone()
    assert all(getattr(c, f) is not None for f in ('labels', 'colour', 'confidence', 'image', 'frame', 'overlay'))
