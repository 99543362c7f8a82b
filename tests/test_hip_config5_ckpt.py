"""GPU tier: BASELINE config 5 (T = 20 long-sequence recurrent encoder; config/settings_DSEC.yaml:7 makes T = 20 the reference
default) and SURVEY 8(f)3 (checkpoint -> HIP path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def _e2vid(cfg, sd):
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    m = E2VIDRecurrent(dict(cfg))
    m.load_state_dict(sd)
    return m.cuda().eval()


def _flat(states):
    """state tensors of all levels: (h, c) pairs of a ConvLSTM, h of a ConvGRU"""
    out = []
    for s in states:
        out += list(s) if isinstance(s, (tuple, list)) else [s]
    return out


@pytest.mark.parametrize('rtype', ['convlstm', 'convgru'])
def test_config5_T20_recurrent_state_drift_vs_oracle(rtype):
    """T = 20 recurrent steps at 96x128 (B = 2, C = 2) against the oracle, step by step: the ConvLSTM hidden / cell states
    (ConvGRU: hidden states -- BASELINE config 5 names the ConvGRU variant) of all three levels and the last step's latents +
    reconstruction.  fp32 arithmetic: 2e-4 at every step (the per-sequence goldens state 1e-4 after 5 steps).  bf16 arithmetic
    (config 5 itself): the state drift is BOUNDED, not growing with T -- the gates are contractive (sigmoid / tanh) -- stated
    tolerance 2e-2 of the state scale at every step.  The bf16 run is repeated with lean steps (t < T-1: no fp32 NCHW state is
    written, the BF16_C8 copies and channel-blocked fp32 states carry the recurrence): bit-identical final outputs."""
    from ess_amd import hip
    B, T, C, H, W = 2, 20, 2, 96, 128
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd = O.synth_state_dict(O.e2vid_param_shapes(cfg), 71)
    ev, _, _, _ = O.synth_batch(B, T, C, H, W, 11, seed=13)
    # oracle trajectory
    ref_states, states = [], None
    with torch.no_grad():
        for t in range(T):
            x = O.event_normalize(ev[:, t * C:(t + 1) * C])
            img, states, lat = O.e2vid_step(sd, cfg, x, states, encoder_only=t < T - 1)
            ref_states.append([s.clone() for s in _flat(states)])
    for mode, tol in (('fp32', 2e-4), ('bf16', 2e-2), ('mixed', 3e-3)):  # (mixed: half operands, pairs at the deepest level -- measured 2-4e-4)
        hip.set_compute(mode)
        try:
            model = _e2vid(cfg, sd)
            st, drift = None, []
            with torch.no_grad():
                for t in range(T):
                    x = hip.event_normalize(ev[:, t * C:(t + 1) * C].contiguous().cuda())
                    out, st, latent = model(x, st, encoder_only=t < T - 1)
                    e = max(_relerr(a, b) for a, b in zip(_flat(st), ref_states[t]))
                    drift.append(e)
                    assert e < tol, (mode, t, e)
            print(f'config5 T=20 {rtype} {mode}: state drift step 1 {drift[0]:.2e}, step 5 {drift[4]:.2e}, step 10 {drift[9]:.2e}, '
                  f'step 20 {drift[19]:.2e}')
            assert _relerr(out, img) < tol
            for k in (2, 4, 8):
                assert _relerr(latent[k], lat[k]) < tol, (mode, k)
            if mode == 'mixed':
                assert max(drift[10:]) < 3 * max(drift[:10]) + 1e-4
            if mode == 'bf16':  # bounded, not accumulating: the second half of the sequence is no worse than 3x the first
                assert max(drift[10:]) < 3 * max(drift[:10]) + 1e-3
                st2 = None
                with torch.no_grad():
                    for t in range(T):
                        x = hip.event_normalize(ev[:, t * C:(t + 1) * C].contiguous().cuda())
                        out2, st2, latent2 = model(x, st2, encoder_only=t < T - 1, lean=t < T - 1)
                assert torch.equal(out2, out) and all(torch.equal(latent2[k], latent[k]) for k in (2, 4, 8))
                assert all(torch.equal(a, b) for a, b in zip(_flat(st2), _flat(st)))
        finally:
            hip.set_compute('fp32')


@pytest.mark.parametrize('rtype,C,H', [('convlstm', 2, 480), ('convgru', 2, 480), ('convlstm', 5, 440)])
def test_config5_T20_full_size_lean_steps_and_step(rtype, C, H):
    _config5_T20(rtype, C, H, 'bf16')


@pytest.mark.parametrize('rtype,C,H', [('convlstm', 2, 480), ('convgru', 2, 480)])
def test_config5_T20_full_size_lean_steps_and_step_mixed(rtype, C, H):
    """the same in the mixed configuration: the deepest level's [hi | lo] pair on the last 3 of the 20 steps"""
    _config5_T20(rtype, C, H, 'mixed')


def _config5_T20(rtype, C, H, mode):
    """Config 5 shape on one GPU (B = 8, T = 20, 2x480x640, bf16; ConvLSTM and the ConvGRU variant the config names) and the
    reference's OWN default shape (nr_events_data 20, nr_temporal_bins 5, 440x640: config/settings_DSEC.yaml:6-7,15 -- 55-row
    eighth-resolution planes, 5-channel head): the 19 lean encoder-only steps + the full last step are deterministic, finite, equal
    to the same sequence run with every fp32 state materialised, and one UDA train step over the T = 20 sequence runs and moves the
    loss."""
    from ess_amd import hip
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.training.ess_trainer import ESSModel
    from ess_amd.training.synthetic import make_batch
    B, T, W, K = 8, 20, 640, 11
    hip.set_compute(mode)
    try:
        cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
        sd = O.synth_state_dict(O.e2vid_param_shapes(cfg), 72)
        ev, img, lab_a, lab_b = make_batch(B, T, C, H, W, K, seed=900, device='cuda')

        def run(lean):
            model = _e2vid(cfg, sd)
            st = None
            with torch.no_grad():
                for t in range(T):
                    last = t == T - 1
                    x = hip.event_normalize(ev[:, t * C:(t + 1) * C].contiguous())
                    out, st, lat = model(x, st, encoder_only=not last, lean=lean and not last)
            return [out] + [lat[k] for k in (2, 4, 8)] + [s[1] if isinstance(s, tuple) else s for s in st]

        a, b, c = run(True), run(True), run(False)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), 'not deterministic'
        assert all(torch.equal(x, y) for x, y in zip(a, c)), 'lean recurrent steps change the result'
        assert all(torch.isfinite(x).all() for x in a)
        del a, b, c
        torch.manual_seed(6)
        tr = ESSModel(synthetic_settings('ess', 'DSEC_events', (H, W), K, B, T, C, e2vid={'recurrent_block_type': rtype}))
        l0 = tr.train_step([[img, lab_a], [ev, lab_b]])[2].item()
        l1 = tr.train_step([[img, lab_a], [ev, lab_b]])[2].item()
        assert l0 == l0 and l1 == l1 and abs(l0) < 1e6 and l0 != l1
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_checkpoint_to_hip_forward(tmp_path, mode):
    """an E2VID checkpoint in the reference's file layout (e2vid/utils/loading_utils.py:5-38) -> load_model ->
    HIP forward, and an ESS checkpoint written by CheckpointSaver (utils/saver.py:15-60) -> restored decoder -> HIP forward,
    both against the oracle on the same state_dict."""
    from ess_amd import hip
    from ess_amd.e2vid.utils.loading_utils import load_model
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.utils.saver import CheckpointSaver
    B, T, C, H, W, K = 1, 3, 2, 64, 96, 6
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type='convlstm', norm='BN')
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 81)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 82, decoder_style=True)
    torch.save({'arch': 'E2VIDRecurrent', 'model': dict(cfg), 'state_dict': sd_e}, tmp_path / 'E2VID_lightweight.pth.tar')
    ev, _, _, lab = O.synth_batch(B, T, C, H, W, K, seed=21)
    ref_logits, ref_lbl, _ = O.validate_batch(sd_e, cfg, sd_d, ev, lab, T, K)
    hip.set_compute(mode)
    try:
        model, _ = load_model(str(tmp_path / 'E2VID_lightweight.pth.tar'))
        model = model.cuda().eval()
        dec0 = SemSegE2VID(256, K, skip_connect=True, skip_type='concat')
        dec0.load_state_dict(sd_d)
        saver = CheckpointSaver(str(tmp_path / 'ckpt'))
        saver.save_checkpoint({'back_end': dec0}, {}, 3, 17, 2, 2)
        dec = SemSegE2VID(256, K, skip_connect=True, skip_type='concat')
        saver.load_checkpoint({'back_end': dec}, {}, checkpoint_file=str(tmp_path / 'ckpt' / 'Epoch_3.pt'), load_optimizer=False)
        dec = dec.cuda().eval()
        st = None
        with torch.no_grad():
            for t in range(T):
                x = hip.event_normalize(ev[:, t * C:(t + 1) * C].contiguous().cuda())
                _, st, latent = model(x, st, encoder_only=True)
            logits = dec(latent)[1]
        rng = (ref_logits.max() - ref_logits.min()).item()
        err = (logits.cpu() - ref_logits).abs().max().item()
        print(f'checkpoint -> HIP ({mode}): max|dlogit| {err:.2e} of range {rng:.3f}')
        assert err < (1e-3 if mode == 'fp32' else 5e-2 * rng)
    finally:
        hip.set_compute('fp32')
