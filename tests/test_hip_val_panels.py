"""GPU tier of the trainers' validation panels (BaseTrainer.vis_panels, img_summaries, visualizeSensorA / visualizeSensorB of ESSModel and
ESSSupervisedModel; reference training/base_trainer.py:455-458,551-554, ess_trainer.py:546-603, ess_supervised_trainer.py:294-333) on the
synthetic loaders at the smallest size the trainer tests use (32 x 48), with a 6-batch validation loader: the reference's three tags per
sensor, the panel shapes, the label rows against tests/viz_ref.py applied to the argmax of the decoder's logits (caught by a forward
hook), and the validation summary with and without panels."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import viz_ref as V  # noqa: E402

H, W, K, B = 32, 48, 6, 2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tile(panel, k):
    y, x = V.grid_slot(k, 4, H, W)
    return panel[:, y:y + H, x:x + W]


def _run(tr):
    """validationEpochs without and with panels on the same trainer -> (summary off, summary on, logits of every decoder call of the
    second run)"""
    assert tr.vis_panels is False and tr.last_val_panels == {}
    tr.validationEpochs()
    off = copy.deepcopy(tr.last_val_summary)
    assert tr.last_val_panels == {}
    calls = []
    hook = tr.task_backend.register_forward_hook(lambda m, i, o: calls.append(o[1].detach().clone()))
    tr.vis_panels = True
    try:
        tr.validationEpochs()
    finally:
        hook.remove()
        tr.vis_panels = False
    return off, copy.deepcopy(tr.last_val_summary), calls


def test_uda_trainer_validation_panels():
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.training.ess_trainer import ESSModel
    st = synthetic_settings('ess', 'DSEC_events', (H, W), K, B, 2, 2, val_steps=6)
    tr = ESSModel(st)
    off, on, calls = _run(tr)
    assert off == on  # (exactly: the panels do not disturb the step)
    tags = {f'val_{name}/reconst_input_{name}_{i}' for name in ('gray', 'events') for i in range(3)}
    assert set(tr.last_val_panels) == tags
    assert len(calls) == 6 + 2 * 6
    col = V.colour_table(st.semseg_color_map)
    batches_a, batches_b = list(tr.val_loader_sensor_a), list(tr.val_loader_sensor_b)
    for i in range(3):
        b = 2 * i + 1  # (6 batches, one panel every second batch: the reference's index rule)
        pa = tr.last_val_panels[f'val_gray/reconst_input_gray_{i}']
        assert pa.is_cuda and pa.dtype == torch.float32 and tuple(pa.shape) == (3, 2 * (H + 2) + 2, 4 * (W + 2) + 2)
        pa = pa.cpu().numpy()
        img, gt = batches_a[b][0].cpu().numpy(), batches_a[b][1].cpu().numpy()
        pred = calls[b].argmax(1).cpu().numpy()
        want = V.panel([('gray', img), ('semseg', pred), ('semseg', gt)], 4, col)
        assert np.array_equal(_bits(pa), _bits(want)), i
        for j in range(B):
            assert np.array_equal(_bits(_tile(pa, B + j)), _bits(V.semseg(pred[j:j + 1], col)[0]))
        pb = tr.last_val_panels[f'val_events/reconst_input_events_{i}']
        assert tuple(pb.shape) == (3, 3 * (H + 2) + 2, 4 * (W + 2) + 2)  # five rows of two tiles, four per grid row
        pb = pb.cpu().numpy()
        ev, gt = batches_b[b][0].cpu().numpy(), batches_b[b][1].cpu().numpy()
        pred, cyc = calls[6 + 2 * b].argmax(1).cpu().numpy(), calls[6 + 2 * b + 1].argmax(1).cpu().numpy()
        for r, lab in ((2, pred), (3, cyc), (4, gt)):
            for j in range(B):
                assert np.array_equal(_bits(_tile(pb, r * B + j)), _bits(V.semseg(lab[j:j + 1], col)[0])), (i, r, j)
        # the event row: the LAST slice's two channels as a histogram tile (createRGBImage's dispatch on two channels)
        assert np.array_equal(_bits(_tile(pb, 0)), _bits(V.events(ev[:1, -2:], 'histogram')[0]))
        fake = _tile(pb, B)
        assert np.array_equal(fake[0], fake[1]) and np.array_equal(fake[0], fake[2]) and len(np.unique(fake)) > 1  # (a gray image)


def test_supervised_trainer_validation_panels():
    """four event channels per slice: the signed tile in its unit form (separate_pol_b is off)"""
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.training.ess_supervised_trainer import ESSSupervisedModel
    st = synthetic_settings('ess_supervised', 'DDD17_events', (H, W), K, B, 2, 4, train_on_event_labels=True, val_steps=6)
    tr = ESSSupervisedModel(st)
    off, on, calls = _run(tr)
    assert off == on
    assert set(tr.last_val_panels) == {f'val_events/reconst_input_events_{i}' for i in range(3)}
    assert len(calls) == 6
    col = V.colour_table(st.semseg_color_map)
    batches = list(tr.val_loader_sensor_b)
    for i in range(3):
        b = 2 * i + 1
        p = tr.last_val_panels[f'val_events/reconst_input_events_{i}']
        assert tuple(p.shape) == (3, 2 * (H + 2) + 2, 4 * (W + 2) + 2)  # events | prediction | ground truth | img_fake
        p = p.cpu().numpy()
        ev, gt = batches[b][0].cpu().numpy(), batches[b][1].cpu().numpy()
        pred = calls[b].argmax(1).cpu().numpy()
        for r, lab in ((1, pred), (2, gt)):
            for j in range(B):
                assert np.array_equal(_bits(_tile(p, r * B + j)), _bits(V.semseg(lab[j:j + 1], col)[0])), (i, r, j)
        for j in range(B):
            assert np.array_equal(_bits(_tile(p, j)), _bits(V.events(ev[j:j + 1, -4:], 'signed', unit=True)[0])), (i, j)
        fake = _tile(p, 3 * B)
        assert np.array_equal(fake[0], fake[1]) and len(np.unique(fake)) > 1
        assert (p[:, :2] == 0).all() and (p[:, :, :2] == 0).all()  # (the padding)
