"""CPU tier: the C-ABI library loads and exports every symbol include/ess_hip.h declares (no compute without a GPU),
host-side planning/validation logic, RAdam rectification schedule, settings parsing, and the data-parallel gradient
reducer over gloo with world_size 2."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


def test_library_exports_every_declared_symbol(built_lib):
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    declared = set(re.findall(r'\b(ess_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 20
    lib = ctypes.CDLL(built_lib)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    from ess_amd import hip
    assert set(hip.EXPORTS) == declared


def test_conv_plan_and_validation_on_host(built_lib):
    from ess_amd import hip
    sp = hip.conv_spec(8, 240, 320, 64, 64, 256, 3, 1, 1, epi=hip.EPI_LSTM, hidden=64)
    assert (sp.H_out, sp.W_out) == (240, 320)
    assert sp.plan.cout_tile == 64 and sp.plan.ck == 8 and sp.plan.n_chunks == 16 and sp.plan.n_cout_tiles == 4
    assert sp.plan.packed_elems == 256 * 128 * 9 and sp.plan.packed_bytes == 4 * sp.plan.packed_elems and sp.plan.lds_bytes <= 64 * 1024
    sb = hip.conv_spec(8, 240, 320, 64, 64, 256, 3, 1, 1, epi=hip.EPI_LSTM, hidden=64, compute=hip.COMPUTE_BF16)
    assert sb.plan.ck == 16 and sb.plan.packed_bytes == 2 * sb.plan.packed_elems and sb.plan.lds_bytes <= 64 * 1024
    head = hip.conv_spec(2, 200, 352, 2, 0, 32, 5, 1, 2, act=hip.ACT_RELU)
    assert head.plan.ck == 2 and head.plan.cout_tile == 32
    assert hip.conv_spec(1, 8, 8, 3, 0, 8, 3, 1, 1).plan.ck == 8  # narrow inputs are zero-padded to the chunk
    small = hip.conv_spec(1, 24, 40, 32, 0, 11, 1, 1, 0)  # 11 classes padded to a 32-row tile
    assert small.plan.rows_padded == 32
    with pytest.raises(hip.EssHipError, match='ksize'):
        hip.conv_spec(1, 8, 8, 4, 0, 4, 4, 1, 1)
    with pytest.raises(hip.EssHipError, match='LSTM'):
        hip.conv_spec(1, 8, 8, 4, 4, 12, 3, 1, 1, epi=hip.EPI_LSTM, hidden=4)
    # ESS_COMPUTE_F16 (the mixed configuration's forward arithmetic) plans exactly like bf16: same tiles, chunks and pack sizes
    sh = hip.conv_spec(8, 240, 320, 64, 64, 256, 3, 1, 1, epi=hip.EPI_LSTM, hidden=64, compute=hip.COMPUTE_F16)
    assert (sh.plan.ck, sh.plan.cout_tile, sh.plan.packed_bytes, sh.plan.lds_bytes) == (sb.plan.ck, sb.plan.cout_tile, sb.plan.packed_bytes, sb.plan.lds_bytes)
    # ... a [hi | lo] x operand is 2 C stored channels, a [hi | lo] copy of h' is requested through `act`
    sx = hip.conv_spec(8, 60, 80, 512, 256, 1024, 3, 1, 1, epi=hip.EPI_LSTM, hidden=256, act=hip.LSTM_H_HILO, compute=hip.COMPUTE_F16)
    assert sx.plan.n_chunks == 48
    lib = hip.lib()
    d = sh.desc_fmt(hip.FMT_BF16_C8, hip.FMT_F32_NCHW, hip.FMT_F32_NCHW)  # (half-operand convolutions read F16_C8, never BF16_C8)
    plan = hip.EssConvPlan()
    assert lib.ess_conv2d_plan(ctypes.byref(d), ctypes.byref(plan)) == -22 and b'F16_C8' in lib.ess_last_error()
    lin = hip.conv_spec(2, 24, 40, 64, 0, 64, 3, 1, 1, compute=hip.COMPUTE_F16)
    assert lib.ess_conv2d_plan(ctypes.byref(lin.desc_fmt(hip.FMT_F16_C8, hip.FMT_F16_C8_HILO, hip.FMT_F32_NCHW)), ctypes.byref(plan)) == 0
    with pytest.raises(hip.EssHipError, match='HILO'):  # an output format of ESS_COMPUTE_F16 only
        bad = hip.conv_spec(2, 24, 40, 64, 0, 64, 3, 1, 1, compute=hip.COMPUTE_BF16)
        hip._check(lib.ess_conv2d_plan(ctypes.byref(bad.desc_fmt(hip.FMT_BF16_C8, hip.FMT_F16_C8_HILO, hip.FMT_F32_NCHW)), ctypes.byref(plan)), 'plan')
    with pytest.raises(hip.EssHipError, match='pooled'):
        hip.conv_spec(2, 24, 40, 64, 0, 64, 3, 1, 1, act=hip.ACT_SUMPOOL2, compute=hip.COMPUTE_F16)
    assert lib.ess_version() == 110


def test_hilo_output_plans_keep_whole_channel_tiles(built_lib):
    """A [hi | lo] (ESS_FMT_F16_C8_HILO) output's lo blocks are written by the straight-line epilogue only, which needs every channel of
    a workgroup's tile: every HILO-output descriptor the plan accepts has C_out a multiple of its plan's cout_tile, every other one is
    refused with a message.  The sweep crosses C_out with doubled [hi | lo] sources on both sides of the 512 input channels at which
    the plan moves to 128-channel tiles."""
    from ess_amd import hip
    lib = hip.lib()
    plan = hip.EssConvPlan()
    accepted, refused = set(), set()
    for k, s, p in ((3, 1, 1), (5, 2, 2), (1, 1, 0), (3, 2, 1)):
        for C0, C1 in ((256, 0), (512, 0), (384, 128), (256, 256), (512, 256), (128, 64), (64, 0)):
            for Co in (11, 32, 64, 96, 128, 192, 256, 320, 384, 512):
                spec = hip.conv_spec(2, 24, 40, C0, C1, Co, k, s, p, compute=hip.COMPUTE_F16)
                d = spec.desc_fmt(hip.FMT_F16_C8, hip.FMT_F16_C8_HILO, hip.FMT_F32_NCHW)
                rc = lib.ess_conv2d_plan(ctypes.byref(d), ctypes.byref(plan))
                if rc == 0:
                    assert Co % plan.cout_tile == 0 and plan.cout_tile == spec.plan.cout_tile, (k, s, C0, C1, Co, plan.cout_tile)
                    accepted.add((k, C0 + C1, Co))
                else:
                    assert rc == -22 and b'[hi | lo] output' in lib.ess_last_error(), (k, s, C0, C1, Co, lib.ess_last_error())
                    refused.add((k, C0 + C1, Co))
    # the edge itself: C_out = 320 behind a doubled 256-channel source (512 stored channels: 128-channel tiles) is refused, C_out = 256
    # (the product's shape) and C_out = 192 / 320 below 512 input channels (64-channel tiles) are planned
    assert (3, 512, 320) in refused and (3, 768, 320) in refused and (3, 512, 192) in accepted
    assert {(3, 512, 256), (3, 256, 192), (3, 256, 320), (3, 192, 192)} <= accepted
    assert (3, 256, 11) in refused and (3, 256, 96) in refused  # (C_out % 64)
    # the product's decoder asks for a pair output only where its plan allows one (functional.Conv2dFn falls back to one half copy)
    fspec = hip.conv_spec(8, 60, 80, 512, 0, 320, 3, 1, 1, compute=hip.COMPUTE_F16)
    assert 320 % fspec.plan.cout_tile != 0


_F32, _BF16, _X3 = 0, 1, 2   # ESS_COMPUTE_*
_NCHW, _C8 = 0, 1            # ESS_FMT_F32_NCHW, ESS_FMT_BF16_C8
# what runs, compute, X format, dY format, (N, H_in, W_in), (C0, C1, C_out), (k, stride, pad), (mode0, mode1), workspace bytes.
# One row per weight-gradient kernel and per special case of the plan.  The byte counts were recorded from the library BEFORE kernel
# choice moved into one function (ess_version 110): they pin nsplit and the slab size of every route, and the split-operand layout.
_WGRAD_PLANS = [
    ('fp32 tile 3x3 / stride 1', _F32, _NCHW, _NCHW, (2, 16, 24), (32, 0, 32), (3, 1, 1), (0, 0), 443904),
    ('fp32 tile 3x3 / stride 2', _F32, _NCHW, _NCHW, (2, 16, 24), (32, 0, 64), (3, 2, 1), (0, 0), 295936),
    ('fp32 tile 1x1 / stride 1', _F32, _NCHW, _NCHW, (2, 16, 24), (32, 0, 64), (1, 1, 0), (0, 0), 101376),
    ('fp32 tile 1x1 / stride 2', _F32, _NCHW, _NCHW, (2, 16, 24), (64, 0, 128), (1, 2, 0), (0, 0), 133120),
    ('fp32 tile, concat with an up-sampled first source', _F32, _NCHW, _NCHW, (2, 16, 24), (64, 32, 32), (3, 1, 1), (1, 0), 1328640),
    ('fp32 tile, ragged channels, odd extents', _F32, _NCHW, _NCHW, (1, 17, 30), (12, 0, 17), (3, 1, 1), (0, 0), 66708),
    ('fp32 tile at the 64 MB slab cap', _F32, _NCHW, _NCHW, (2, 64, 96), (512, 0, 512), (3, 1, 1), (0, 0), 66074624),
    ('7x7 stem', _F32, _NCHW, _NCHW, (2, 32, 48), (1, 0, 64), (7, 2, 3), (0, 0), 153600),
    ('7x7 stem, BF16_C8 dY', _BF16, _NCHW, _C8, (2, 32, 48), (1, 0, 64), (7, 2, 3), (0, 0), 153600),
    ('fp32-staged bf16 3x3, general form (W % 8 != 0)', _BF16, _NCHW, _NCHW, (1, 17, 30), (12, 8, 40), (3, 1, 1), (0, 0), 144800),
    ('fp32-staged bf16 3x3, general form (zero-upsampled source)', _BF16, _NCHW, _NCHW, (2, 16, 24), (32, 0, 32), (3, 1, 1), (2, 0), 295936),
    ('fp32-staged bf16 3x3, fast form', _BF16, _NCHW, _NCHW, (2, 16, 24), (20, 16, 64), (3, 1, 1), (0, 0), 665600),
    ('fp32-staged bf16 1x1', _BF16, _NCHW, _NCHW, (2, 16, 24), (64, 0, 128), (1, 1, 0), (0, 0), 266240),
    ('bf16 1x1 with W % 8 != 0: the fp32 tile kernel', _BF16, _NCHW, _NCHW, (1, 17, 30), (64, 0, 128), (1, 1, 0), (0, 0), 299520),
    ('BF16_C8 LDS-DMA 3x3', _BF16, _C8, _C8, (2, 16, 24), (32, 0, 64), (3, 1, 1), (0, 0), 591872),
    ('BF16_C8 3x3, concat with an up-sampled first source', _BF16, _C8, _C8, (2, 16, 24), (64, 32, 64), (3, 1, 1), (1, 0), 1771520),
    ('BF16_C8 3x3, ragged channels, odd extents', _BF16, _C8, _C8, (1, 17, 30), (12, 0, 40), (3, 1, 1), (0, 0), 104640),
    ('BF16_C8 3x3, output smaller than one pixel tile', _BF16, _C8, _C8, (1, 5, 7), (32, 0, 32), (3, 1, 1), (0, 0), 36992),
    ('BF16_C8 3x3, 512 -> 512', _BF16, _C8, _C8, (2, 64, 96), (512, 0, 512), (3, 1, 1), (0, 0), 37756928),
    ('BF16_C8 3x3 / stride 2 by parity phases', _BF16, _C8, _C8, (2, 16, 24), (64, 0, 128), (3, 2, 1), (0, 0), 590848),
    ('BF16_C8 1x1 / stride 1', _BF16, _C8, _C8, (2, 16, 24), (64, 0, 128), (1, 1, 0), (0, 0), 266240),
    ('BF16_C8 1x1 / stride 2', _BF16, _C8, _C8, (2, 16, 24), (64, 0, 128), (1, 2, 0), (0, 0), 66560),
    ('small 1x1', _F32, _NCHW, _NCHW, (2, 17, 30), (64, 0, 11), (1, 1, 0), (0, 0), 22880),
    ('small 1x1 at its 1024-slab limit', _F32, _NCHW, _NCHW, (8, 120, 160), (64, 0, 16), (1, 1, 0), (0, 0), 4259840),
    ('small 1x1 MFMA', _F32, _NCHW, _NCHW, (2, 16, 24), (32, 0, 11), (1, 1, 0), (0, 0), 4356),
    ('small 1x1 MFMA at its 512-slab limit', _F32, _NCHW, _NCHW, (8, 120, 160), (32, 0, 6), (1, 1, 0), (0, 0), 405504),
    ('small 1x1, BF16_C8 X and fp32 dY', _BF16, _C8, _NCHW, (2, 16, 24), (32, 0, 11), (1, 1, 0), (0, 0), 8712),
    ('bf16x3 through BF16_C8 copies', _X3, _NCHW, _NCHW, (2, 16, 24), (32, 0, 64), (3, 1, 1), (0, 0), 886784),
    ('bf16x3 through BF16_C8 copies, concat with an up-sampled first source', _X3, _NCHW, _NCHW, (2, 16, 24), (64, 32, 64), (3, 1, 1), (1, 0), 2115584),
    ('bf16x3 on the fp32-staged kernels (C0 % 8 != 0), fast form', _X3, _NCHW, _NCHW, (2, 16, 24), (20, 16, 64), (3, 1, 1), (0, 0), 665600),
    ('bf16x3 on the fp32-staged kernels (C0 % 8 != 0), general form', _X3, _NCHW, _NCHW, (1, 17, 30), (12, 8, 40), (3, 1, 1), (0, 0), 144800),
    ('bf16x3 1x1: exact fp32', _X3, _NCHW, _NCHW, (2, 16, 24), (32, 0, 64), (1, 1, 0), (0, 0), 101376),
    ('bf16x3 3x3 / stride 2: exact fp32', _X3, _NCHW, _NCHW, (2, 16, 24), (32, 0, 64), (3, 2, 1), (0, 0), 295936),
]


def _wgrad_desc(hip, comp, fx, fy, nhw, ch, ksp, modes=(0, 0)):
    (N, H, W), (C0, C1, Co), (k, s, p) = nhw, ch, ksp
    return hip.EssConvDesc(N, H, W, C0, C1, modes[0], modes[1], Co, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, k, s, p,
                           hip.EPI_LINEAR, hip.ACT_NONE, 0, 0, comp, fx, fx, fy, _NCHW)


@pytest.mark.parametrize('row', _WGRAD_PLANS, ids=[r[0] for r in _WGRAD_PLANS])
def test_wgrad_plan_workspace_is_pinned(built_lib, row):
    from ess_amd import hip
    assert (hip.COMPUTE_FP32, hip.COMPUTE_BF16, hip.COMPUTE_BF16X3, hip.FMT_F32_NCHW, hip.FMT_BF16_C8) == (_F32, _BF16, _X3, _NCHW, _C8)
    assert os.environ.get('ESS_X3_WGRAD_C8', '1')[:1] != '0'  # (the switch moves bf16x3 to the fp32-staged kernels: other byte counts)
    what, comp, fx, fy, nhw, ch, ksp, modes, nbytes = row
    d = _wgrad_desc(hip, comp, fx, fy, nhw, ch, ksp, modes)
    assert hip.lib().ess_conv2d_wgrad_workspace(ctypes.byref(d)) == nbytes, (what, hip.lib().ess_last_error())


@pytest.mark.parametrize('what, args, fragment', [
    ('a BF16_C8 5x5', (_BF16, _C8, _C8, (2, 16, 24), (32, 0, 32), (5, 1, 2)), 'k=5 with C_in=32 unsupported'),
    ('a BF16_C8 concat whose first source is not whole blocks', (_BF16, _C8, _C8, (2, 16, 24), (20, 16, 64), (3, 1, 1)),
     'the first BF16_C8 source of a concat must have a multiple of 8 channels'),
    ('an F16 compute type', (3, _NCHW, _NCHW, (2, 16, 24), (32, 0, 32), (3, 1, 1)), 'bad compute type'),
    ('BF16_C8 X with fp32 dY beyond 32 channels', (_BF16, _C8, _NCHW, (2, 16, 24), (64, 0, 11), (1, 1, 0)),
     'wgrad(BF16_C8 X, fp32 dY): the 1x1 head only'),
])
def test_wgrad_plan_refusals(built_lib, what, args, fragment):
    from ess_amd import hip
    assert hip.COMPUTE_F16 == 3
    lib = hip.lib()
    assert lib.ess_conv2d_wgrad_workspace(ctypes.byref(_wgrad_desc(hip, *args))) == 0, what
    assert fragment.encode() in lib.ess_last_error(), (what, lib.ess_last_error())
    # ... and the call itself refuses before it touches a pointer
    assert lib.ess_conv2d_wgrad(ctypes.byref(_wgrad_desc(hip, *args)), None, None, None, None, None, 0, None, ctypes.c_size_t(0), None) == -22
    assert fragment.encode() in lib.ess_last_error()


def test_product_refuses_cpu_tensors(built_lib):
    from ess_amd import hip
    with pytest.raises(hip.EssHipError, match='no CPU path'):
        hip.event_normalize(torch.zeros(1, 2, 4, 4))


def test_missing_library_is_loud(monkeypatch, built_lib):
    from ess_amd import hip
    monkeypatch.setattr(hip, '_lib', None)
    monkeypatch.setattr(hip, 'LIB_PATH', '/nonexistent/libess_hip.so')
    with pytest.raises(hip.EssHipError, match='no CPU or eager fallback'):
        hip.lib()


def test_radam_rectification_matches_oracle():
    from oracle import ess_oracle as O
    from ess_amd.utils.radam import RAdam
    for step in range(1, 40):
        assert RAdam.rectification(step, 0.0, 0.999) == O.radam_step_size(step, 0.0, 0.999)
    assert RAdam.rectification(5, 0.0, 0.999)[0] < 5 <= RAdam.rectification(6, 0.0, 0.999)[0]


def test_state_dict_layout_matches_reference_tables():
    """The product modules expose exactly the reference's state_dict keys/shapes (pinned through the oracle tables,
    which tests/golden/make_golden.py asserts against the imported reference)."""
    from oracle import ess_oracle as O
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.models.style_networks import SemSegE2VID, StyleEncoderE2VID
    for rec in ('convlstm', 'convgru'):
        for norm in ('BN', 'none', 'IN'):
            for up in (True, False):
                cfg = O.e2vid_config(num_bins=5, recurrent_block_type=rec, norm=norm, use_upsample_conv=up, base_num_channels=8)
                got = {k: tuple(v.shape) for k, v in E2VIDRecurrent(dict(cfg)).state_dict().items()}
                assert got == {k: tuple(v) for k, v in O.e2vid_param_shapes(cfg).items()}, (rec, norm, up)
    for skip in (True, False):
        got = {k: tuple(v.shape) for k, v in SemSegE2VID(256, 11, skip, 'concat' if skip else 'sum').state_dict().items()}
        assert got == {k: tuple(v) for k, v in O.semseg_param_shapes(256, 11, skip).items()}
    got = {k: tuple(v.shape) for k, v in StyleEncoderE2VID(1, True).state_dict().items()}
    assert got == {k: tuple(v) for k, v in O.style_encoder_param_shapes(1).items()}


def test_settings_parses_reference_yaml_schema(tmp_path):
    import yaml
    from ess_amd.config.settings import Settings
    ref_yaml = {
        'dataset': {'name_a': 'Cityscapes_gray', 'name_b': 'DSEC_events',
                    'DSEC_events': {'dataset_path': '/none', 'shape': [440, 640], 'nr_events_data': 20,
                                    'nr_events_files_per_data': None, 'fixed_duration': False, 'delta_t_per_data': 50,
                                    'require_paired_data_train': False, 'require_paired_data_val': True,
                                    'nr_events_window': 100000, 'event_representation': 'voxel_grid', 'nr_temporal_bins': 5,
                                    'separate_pol': False, 'normalize_event': False},
                    'cityscapes_img': {'dataset_path': '/none', 'shape': [440, 640], 'random_crop': False,
                                       'read_two_imgs': False, 'require_paired_data_train': False,
                                       'require_paired_data_val': False}},
        'task': {'semseg_num_classes': 11}, 'dir': {'log': str(tmp_path)},
        'model': {'model_name': 'ess', 'skip_connect_encoder': True, 'skip_connect_task': True,
                  'skip_connect_task_type': 'concat', 'data_augmentation_train': True, 'train_on_event_labels': False},
        'optim': {'batch_size_a': 8, 'batch_size_b': 8, 'lr_front': '5e-4', 'lr_back': '5e-4', 'lr_decay': 1, 'num_epochs': 50,
                  'val_epoch_step': 5, 'weight_task_loss': 1, 'weight_cycle_pred_loss': 1, 'weight_cycle_emb_loss': 1,
                  'weight_cycle_task_loss': 1, 'task_loss': ['dice', 'cross_entropy']},
        'checkpoint': {'save_checkpoint': True, 'resume_training': False, 'load_pretrained_weights': False,
                       'resume_file': None, 'pretrained_file': None},
        'hardware': {'num_cpu_workers': 8, 'gpu_device': 0},
        'synthetic': {'enabled': True, 'img_size': [480, 640], 'nr_events_data': 5, 'nr_temporal_bins': 2},
    }
    p = tmp_path / 's.yaml'
    p.write_text(yaml.safe_dump(ref_yaml))
    s = Settings(str(p), generate_log=False)
    assert s.model_name == 'ess' and s.dataset_name_b == 'DSEC_events' and s.semseg_num_classes == 11
    assert s.nr_events_data_b == 5 and s.input_channels_b == 2 and s.img_size_b == [480, 640]
    assert s.weight_KL_loss == 1.0 and s.weight_cycle_loss == 1.0 and s.lr_front == 5e-4
    assert len(s.semseg_class_names) == 11 and s.semseg_ignore_label == 255
    ref_yaml['synthetic']['enabled'] = False
    p.write_text(yaml.safe_dump(ref_yaml))
    with pytest.raises(AssertionError):  # dataset dirs must exist, as in the reference
        Settings(str(p), generate_log=False)


def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from ess_amd.training import distributed as D
    red = D.GradAllReducer()
    g1 = torch.full((1000,), float(rank + 1))
    g2 = torch.arange(10, dtype=torch.float32) * (rank + 1)
    red.launch(g1)
    red.launch(g2)
    red.wait()
    lin = torch.nn.Linear(4, 3)
    torch.manual_seed(rank)
    with torch.no_grad():
        lin.weight.normal_()
    D.broadcast_module(lin, 0)
    out = torch.cat([g1[:2], g2[:3], lin.weight.flatten()[:2]])
    gathered = [torch.zeros_like(out) for _ in range(world)]
    dist.all_gather(gathered, out)
    if rank == 0:
        ret.put([t.tolist() for t in gathered])
    dist.destroy_process_group()


def test_data_parallel_reducer_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    a, b = res
    assert a == b  # both ranks hold the same averaged gradients and the same broadcast weights
    assert a[0] == pytest.approx(1.5) and a[3] == pytest.approx(1.5 * 1) and a[4] == pytest.approx(1.5 * 2)


def _dp_bucket_worker(rank, world, port, ret):
    """One rank of the trainer-level data-parallel check: a small CPU network, per-rank batch shard, gradients written into a
    flat buffer laid out like ess_amd.utils.radam.RAdam's, reported parameter by parameter in BACKWARD order through
    functional.GRAD_READY_HOOK (as Conv2dFn.backward does), bucketed all-reduce, then compared with the single-process
    gradients of the whole batch."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from types import SimpleNamespace
    from ess_amd import functional as Fn
    from ess_amd.training import distributed as D
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(8, 8, 3, padding=1),
                              torch.nn.Tanh(), torch.nn.Conv2d(8, 4, 1))
    D.broadcast_module(net, 0)
    g = torch.Generator().manual_seed(1)
    x_all, y_all = torch.randn(4, 3, 6, 7, generator=g), torch.randn(4, 4, 6, 7, generator=g)
    loss_fn = lambda out, tgt: ((out - tgt) ** 2).mean()  # noqa: E731  (a per-sample mean: linear in the batch)
    # single-process reference over the whole batch
    ref = torch.autograd.grad(loss_fn(net(x_all), y_all), list(net.parameters()))
    # this rank's shard, gradients into a flat buffer with .grad views (the RAdam layout)
    params = list(net.parameters())
    sizes = [p.numel() for p in params]
    flat = torch.zeros(sum(sizes))
    opt = SimpleNamespace(param_groups=[{'params': params}], flat_grad=flat)
    sh = slice(rank * 2, rank * 2 + 2)
    grads = torch.autograd.grad(loss_fn(net(x_all[sh]), y_all[sh]), params)
    red = D.GradAllReducer()
    red.arm(opt, n_buckets=3)
    assert Fn.GRAD_READY_HOOK is not None
    n_fired = []
    off = sum(sizes)
    for p, k, gp in zip(reversed(params), reversed(sizes), reversed(grads)):  # backward order: last layer first
        off -= k
        flat[off:off + k] = gp.reshape(-1)
        if p.dim() == 4:
            Fn.GRAD_READY_HOOK(p)  # (biases are completed by the same launch as their weight)
        n_fired.append(len(red.pending))
    red.wait()
    assert Fn.GRAD_READY_HOOK is None
    err, off = 0.0, 0
    for k, r in zip(sizes, ref):
        err = max(err, (flat[off:off + k] - r.reshape(-1)).abs().max().item())
        off += k
    if rank == 0:
        ret.put((err, n_fired))
    dist.destroy_process_group()


def test_data_parallel_bucketed_gradients_match_single_process_gloo_world2():
    """SURVEY section 4 / VERDICT r1 #3: averaged per-rank gradients == single-process gradients of the whole batch, through
    the bucketed reducer the trainers use, with the buckets issued from inside the (simulated) backward pass."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_bucket_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    err, n_fired = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert err < 1e-6, err
    # collectives in flight after each parameter of the simulated backward (last layer's bias, weight, ... first layer's weight):
    # the tail bucket goes out as soon as the LAST layer's weight gradient is done -- overlap, not a trailing reduce
    assert n_fired[1] >= 1, n_fired
    assert n_fired[-1] == 2, n_fired


def test_load_model_reads_the_reference_checkpoint_layout(tmp_path):
    """e2vid/utils/loading_utils.py:5-38: {'arch', 'model' | 'config'['model'], 'state_dict'} -> (model, decoder);
    both spellings of the config location, unknown arch refused (no eval())."""
    from oracle import ess_oracle as O
    from ess_amd.e2vid.utils.loading_utils import load_model
    cfg = O.e2vid_config(num_bins=2, recurrent_block_type='convgru', norm='none')
    sd = O.synth_state_dict(O.e2vid_param_shapes(cfg), 5)
    for layout in ('model', 'config'):
        ck = {'arch': 'E2VIDRecurrent', 'state_dict': sd}
        if layout == 'model':
            ck['model'] = dict(cfg)
        else:
            ck['config'] = {'model': dict(cfg)}
        path = tmp_path / f'{layout}.pth.tar'
        torch.save(ck, path)
        model, decoder = load_model(str(path))
        got = model.state_dict()
        assert list(got.keys()) == list(sd.keys())
        assert all(torch.equal(got[k], sd[k]) for k in sd)
        assert model.num_bins == 2 and model.num_encoders == 3
        assert decoder is not None
        # return_task (loading_utils.py:25-37): the checkpoint's resblocks / decoders under a fresh 13-class head; the image
        # prediction layer's weights are not taken over, 'module.'-prefixed keys are accepted
        m2, d2, task = load_model(str(path), return_task=True)
        tsd = task.state_dict()
        assert set(tsd) == set(O.e2vid_task_param_shapes(cfg)) and tsd['unetrecurrent.pred_semseg.1.conv2d.weight'].shape[0] == 13
        shared = [k for k in tsd if k in sd]
        assert shared and all(k.startswith(('unetrecurrent.resblocks.', 'unetrecurrent.decoders.')) for k in shared)
        assert all(torch.equal(tsd[k], sd[k]) for k in shared)
    torch.save({'arch': '__import__("os").system("true")', 'model': dict(cfg), 'state_dict': sd}, tmp_path / 'bad.pth.tar')
    with pytest.raises(ValueError):
        load_model(str(tmp_path / 'bad.pth.tar'))


def test_checkpoint_saver_roundtrip(tmp_path):
    """utils/saver.py:15-60 file layout: Epoch_<n>.pt with one entry per model / optimiser name + epoch, step_count,
    batch sizes; a second set of modules restored from it is identical."""
    from oracle import ess_oracle as O
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.utils.saver import CheckpointSaver

    def make(seed):
        torch.manual_seed(seed)
        dec = SemSegE2VID(256, 6, skip_connect=True, skip_type='concat')
        dec.load_state_dict(O.synth_state_dict(O.semseg_param_shapes(256, 6), seed, decoder_style=True))
        return dec

    a, b = make(1), make(2)
    opt_a = torch.optim.SGD(a.parameters(), lr=0.1, momentum=0.9)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    for p in a.parameters():
        p.grad = torch.ones_like(p)
    opt_a.step()
    saver = CheckpointSaver(str(tmp_path))
    saver.save_checkpoint({'back_end': a}, {'optimizer_back': opt_a}, epoch=3, step_count=17, batch_size_a=8, batch_size_b=8)
    path = tmp_path / 'Epoch_3.pt'
    raw = torch.load(path, map_location='cpu', weights_only=False)
    assert set(raw) == {'back_end', 'optimizer_back', 'epoch', 'step_count', 'batch_size_a', 'batch_size_b'}
    meta = saver.load_checkpoint({'back_end': b}, {'optimizer_back': opt_b}, checkpoint_file=str(path))
    assert meta == {'epoch': 3, 'step_count': 17, 'batch_size_a': 8, 'batch_size_b': 8}
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    ma = opt_a.state_dict()['state'][0]['momentum_buffer']
    mb = opt_b.state_dict()['state'][0]['momentum_buffer']
    assert torch.equal(ma, mb)
    c = make(4)
    saver.load_pretrained_weights({'back_end': c, 'front_sensor_b': None}, ['front_sensor_b', 'back_end'], checkpoint_file=str(path))
    assert all(torch.equal(sa[k], c.state_dict()[k]) for k in sa)


def test_voxel_api_mirrors_reference_and_refuses_cpu(built_lib):
    """ess_amd.datasets mirrors DSEC/dataset/representations.py and datasets/data_util.py by name; without a GPU the
    product refuses to run (no host fallback: the host algorithm lives in oracle/ only)."""
    from ess_amd import hip
    from ess_amd.datasets import data_util
    from ess_amd.datasets.representations import EventRepresentation, VoxelGrid
    vg = VoxelGrid(2, 8, 8, normalize=False)
    assert isinstance(vg, EventRepresentation) and vg.nb_channels == 2
    x = torch.zeros(4)
    with pytest.raises(hip.EssHipError):
        vg.convert(x, x, x, x)
    with pytest.raises(hip.EssHipError):
        data_util.generate_voxel_grid(torch.zeros(4, 4, dtype=torch.float64), (8, 8), 2)
    with pytest.raises(NotImplementedError):
        data_util.generate_input_representation(torch.zeros(4, 4), 'histogram', (8, 8))
    lib = ctypes.CDLL(built_lib)
    lib.ess_voxel_grid_trilinear_workspace.restype = ctypes.c_size_t
    lib.ess_voxel_grid_trilinear_workspace.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    ws = lib.ess_voxel_grid_trilinear_workspace(4_000_000, 40, 480, 640)
    assert 4_000_000 * 16 <= ws < 4_000_000 * 16 + (32 << 20)  # sorted events + per-tile tables (halo table sized for 7 channels)
    assert lib.ess_voxel_grid_trilinear_workspace(0, 40, 480, 640) == 0


def test_radam_state_dict_interop():
    """RAdam.state_dict() carries the reference's per-parameter layout (utils/radam.py:31-47) next to the flat
    buffers; load_state_dict() restores from either, restores param_groups, and refuses anything else."""
    from ess_amd.utils.radam import RAdam
    mk = lambda: [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]  # noqa: E731
    a = RAdam(mk(), lr=1e-3, betas=(0.0, 0.999))
    a._step = 7
    a.exp_avg.copy_(torch.arange(17.0))
    a.exp_avg_sq.copy_(torch.arange(17.0) * 2)
    sd = a.state_dict()
    assert set(sd['state']) == {0, 1} and sd['state'][0]['exp_avg'].shape == (4, 3) and sd['state'][1]['step'] == 7
    b = RAdam(mk(), lr=5e-4, betas=(0.0, 0.999))
    b.load_state_dict(sd)
    assert b._step == 7 and torch.equal(b.exp_avg, a.exp_avg) and b.param_groups[0]['lr'] == 1e-3
    # the reference's own checkpoint layout: per-parameter state only
    ref_sd = {'state': {0: {'step': 3, 'exp_avg': torch.ones(4, 3), 'exp_avg_sq': torch.full((4, 3), 2.0)},
                        1: {'step': 3, 'exp_avg': torch.zeros(5), 'exp_avg_sq': torch.ones(5)}},
              'param_groups': [{'lr': 2e-3, 'betas': (0.0, 0.999), 'eps': 1e-8, 'weight_decay': 0, 'params': [0, 1]}]}
    c = RAdam(mk(), lr=5e-4, betas=(0.0, 0.999))
    c.load_state_dict(ref_sd)
    assert c._step == 3 and c.param_groups[0]['lr'] == 2e-3
    assert torch.equal(c.exp_avg[:12], torch.ones(12)) and torch.equal(c.exp_avg_sq[12:], torch.ones(5))
    with pytest.raises(ValueError):
        c.load_state_dict({'param_groups': ref_sd['param_groups']})
    with pytest.raises(ValueError):
        bad = {'state': {0: dict(ref_sd['state'][0], step=4), 1: ref_sd['state'][1]}, 'param_groups': ref_sd['param_groups']}
        c.load_state_dict(bad)


def test_wrapper_dataset_zipper_vs_reference_golden():
    """ess_amd.datasets.wrapper_dataloader.WrapperDataset against the sequences the reference's class produced
    (tests/golden/zipper.json, generated by tests/golden/make_golden_zipper.py): 48 cases = 4 length pairs x paired / unpaired
    on either side x dataset_len_to_use, two epochs each, including where the epoch-setting loader raises StopIteration."""
    import json
    import sys
    from ess_amd.datasets.wrapper_dataloader import WrapperDataset
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    from zipper_driver import run
    cases = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'zipper.json')))
    assert len(cases) == 48
    for c in cases:
        got = run(WrapperDataset, c['na'], c['nb'], c['paired_a'], c['paired_b'], c['use'])
        assert got == c['log'], (c['na'], c['nb'], c['paired_a'], c['paired_b'], c['use'])


def test_augmentation_params_and_oracle_semantics():
    """SURVEY 8(f)4 host side: parameter rows follow the reference's probabilities / ranges; the oracle's identity parameters
    reproduce a centred pad + crop exactly; flip / integer shift are exact pixel moves."""
    from oracle import ess_oracle as O
    from ess_amd.datasets.augment import draw_params
    g = torch.Generator().manual_seed(0)
    p = draw_params(4000, (256, 512), (200, 352), 0.1, g)
    assert 0.45 < p[:, 0].mean() < 0.55 and (p[:, 1] >= 1).all() and (p[:, 1] <= 1.5).all()
    assert 0.45 < (p[:, 1] > 1).float().mean() < 0.55 and 0.15 < (p[:, 10] > 0).float().mean() < 0.25
    assert (p[:, 6] >= 0).all() and (p[:, 6] <= 56).all() and (p[:, 7] <= 160).all() and p[:, 2].abs().max() <= 51.2
    img = torch.randint(0, 256, (2, 6, 8)).float()
    lab = torch.randint(0, 34, (2, 6, 8))
    ident = draw_params(2, (6, 8), (10, 8), augment=False)
    out, ol = O.augment_image_label(img, lab, ident, 10, 8)
    assert torch.equal((out[:, 0, 2:8] * 255).round(), img) and (out[:, 0, :2] == 0).all() and torch.equal(ol[:, 2:8], lab)
    fl = draw_params(2, (6, 8), (6, 8), augment=False)
    fl[:, 0] = 1
    fl[:, 2] = 0
    out, ol = O.augment_image_label(img, lab, fl, 6, 8)
    assert torch.equal((out[:, 0] * 255).round(), img.flip(-1)) and torch.equal(ol, lab.flip(-1))


def test_augmentation_second_stage_params_and_oracle_semantics():
    """SURVEY 8(f)4, second stage host side: Perspective fires with p = 0.2 and its inverse homography maps the rectangle's corners
    back onto the jittered quadrilateral; OneOf fires with p = 0.5 and its kernels are the three the reference configures
    (Sharpen sums to 1 + alpha (lightness - 1), box = 1/9, motion-blur lines normalised, 2-3 cells); the oracle's identity row is
    the identity, a box blur of a constant image is that constant, a centred-quadrilateral warp keeps the image centre."""
    from oracle import ess_oracle as O
    from ess_amd.datasets.augment import draw_params2, perspective_matrix, _line3
    g = torch.Generator().manual_seed(1)
    H, W = 120, 160
    p = draw_params2(3000, (H, W), g)
    assert 0.17 < p[:, 0].mean() < 0.23 and 0.46 < p[:, 14].mean() < 0.54
    k = p[p[:, 14] > 0][:, 15:24]
    assert ((k.sum(1) - 1).abs() < 1e-5).float().mean() > 0.6  # box and motion kernels sum to 1 exactly, Sharpen to 1 + a*light
    sharp = k[(k[:, 0] < 0)]
    assert len(sharp) > 300 and (sharp[:, 0] <= -0.2).all() and (sharp[:, 0] >= -0.5).all()
    light = (sharp.sum(1) - 1) / (-sharp[:, 0]) + 1  # rows sum to (1 - a) + a * (8 + lightness) - 8 a = 1 + a * (lightness - 1)
    assert (light >= 0.5 - 1e-4).all() and (light <= 1.0 + 1e-4).all()
    motion = k[(k[:, 0] >= 0) & ((k - 1.0 / 9).abs().max(1).values > 1e-6)]
    cells = (motion > 0).sum(1)
    assert len(motion) > 300 and ((cells == 2) | (cells == 3)).all()
    pr = p[p[:, 0] > 0]
    assert (pr[:, 10] <= 1.05 * W).all() and (pr[:, 10] >= 0.5 * W).all() and (pr[:, 11] <= 1.05 * H).all() and (pr[:, 11] >= 0.5 * H).all()
    # inverse homography: rectangle corners -> the (ordered) quadrilateral
    pts = [[10.0, 6.0], [150.0, 9.0], [146.0, 112.0], [5.0, 116.0]]
    minv, mw, mh = perspective_matrix(pts, H, W)
    m = minv.double().view(3, 3)
    for (x, y), q in zip([(0, 0), (mw, 0), (mw, mh), (0, mh)], pts):
        v = m @ torch.tensor([x, y, 1.0], dtype=torch.float64)
        assert abs(v[0] / v[2] - q[0]) < 1e-3 and abs(v[1] / v[2] - q[1]) < 1e-3
    assert _line3(0, 0, 2, 1).tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 0]] and _line3(2, 1, 0, 0).tolist() == _line3(0, 0, 2, 1).tolist()
    assert _line3(1, 0, 1, 2).tolist() == [[0, 1, 0], [0, 1, 0], [0, 1, 0]] and _line3(0, 2, 2, 0).tolist() == [[0, 0, 1], [0, 1, 0], [1, 0, 0]]
    # oracle semantics
    img = torch.randint(0, 256, (2, 1, 12, 16)).float() / 255
    lab = torch.randint(0, 34, (2, 12, 16))
    ident = draw_params2(2, (12, 16), g)
    ident[:, 0], ident[:, 14] = 0, 0
    out, ol = O.augment_perspective_filter(img, lab, ident)
    assert torch.equal((out * 255).round(), (img * 255).round()) and torch.equal(ol, lab)
    box = ident.clone()
    box[:, 14], box[:, 15:24] = 1, 1.0 / 9
    const = torch.full((2, 1, 12, 16), 77 / 255.0)
    assert ((O.augment_perspective_filter(const, None, box)[0] * 255).round() == 77).all()
    # reflect-101 border of the box blur: a horizontal ramp keeps its interior mean, the first column sees (1, 0, 1)
    ramp = (torch.arange(16).float() * 3).view(1, 1, 1, 16).expand(1, 1, 12, 16).contiguous() / 255
    rb = (O.augment_perspective_filter(ramp, None, box[:1])[0] * 255).round()
    assert rb[0, 0, 5, 7].item() == 21 and rb[0, 0, 5, 0].item() == 2


def test_header_enums_match_the_binding():
    """Every enumerator of include/ess_hip.h that ess_amd/hip.py mirrors (ESS_X = n <-> hip.X) carries the same value."""
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    from ess_amd import hip
    pairs = {}
    for body in re.findall(r'enum\s*\{(.*?)\}', header, flags=re.S):
        for name, val in re.findall(r'ESS_([A-Z0-9_]+)\s*=\s*(-?\d+)', body):
            pairs[name] = int(val)
    mirrored = {n: v for n, v in pairs.items() if hasattr(hip, n)}
    assert len(mirrored) >= 15, sorted(mirrored)
    assert {'FMT_F32_NCHW', 'FMT_BF16_C8', 'FMT_F32_C8', 'EPI_LSTM', 'SRC_ZERO_UP2', 'ACT_SUMPOOL2', 'COMPUTE_F16', 'FMT_F16_C8_HILO', 'LSTM_H_HILO', 'GRU_H_HILO'} <= set(mirrored)
    wrong = {n: (v, getattr(hip, n)) for n, v in mirrored.items() if getattr(hip, n) != v}
    assert not wrong, wrong


def test_rccl_process_group_construction_mocked(monkeypatch):
    """No multi-GPU box is available to the build: the RCCL branch of the data-parallel start-up (bench.py --gpus N ->
    distributed.init_for_device) is at least CONSTRUCTED here against a recording stand-in for torch.distributed -- backend
    'nccl', device_id = this rank's device, rendezvous address and the dmabuf-IPC switch in the environment -- and the gradient
    reducer issues averaged asynchronous all-reduces on that backend (ReduceOp.AVG: no post-division kernel)."""
    import torch.distributed as dist
    from ess_amd.training import distributed as D
    calls = {}
    monkeypatch.delenv('ESS_DIST_BACKEND', raising=False)
    monkeypatch.delenv('MASTER_ADDR', raising=False)
    monkeypatch.setattr(dist, 'init_process_group', lambda **kw: calls.update(init=kw))
    dev = torch.device('cuda', 3)
    # without a launcher (no RANK / WORLD_SIZE): refused -- a half-configured launcher must not turn into N independent one-rank groups --
    # unless ESS_DP_FORCE / force_dp asks for the one-rank group (single-GPU box), which rendezvouses through a private file:// store
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(D, '_FORCE', False)
    with pytest.raises(RuntimeError, match='RANK / WORLD_SIZE'):
        D.init_for_device(dev)
    monkeypatch.setattr(D, '_FORCE', True)
    assert D.init_for_device(dev) == 'nccl'
    one = calls['init']
    assert one['backend'] == 'nccl' and one['device_id'] == dev and one['rank'] == 0 and one['world_size'] == 1
    assert one['init_method'].startswith('file://')
    monkeypatch.setattr(D, '_FORCE', False)
    monkeypatch.setenv('RANK', '3')
    monkeypatch.setenv('WORLD_SIZE', '8')
    assert D.init_for_device(dev) == 'nccl'
    assert calls['init'] == {'backend': 'nccl', 'device_id': dev}
    assert os.environ['MASTER_ADDR'] == '127.0.0.1' and os.environ['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'
    monkeypatch.setenv('ESS_DIST_BACKEND', 'gloo')
    assert D.init_for_device(dev) == 'gloo' and calls['init'] == {'backend': 'gloo'}
    # reducer on the (mocked) nccl backend
    class _Work:
        def wait(self):
            calls['waited'] = calls.get('waited', 0) + 1
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 8)
    monkeypatch.setattr(dist, 'get_backend', lambda *a: 'nccl')
    monkeypatch.setattr(dist, 'all_reduce', lambda t, op=None, async_op=False: (calls.setdefault('ops', []).append((t.numel(), op, async_op)), _Work())[1])
    red = D.GradAllReducer()
    g = torch.ones(1000)
    red.launch(g)
    red.wait()
    assert calls['ops'] == [(1000, dist.ReduceOp.AVG, True)] and calls['waited'] == 1
    assert torch.equal(g, torch.ones(1000))  # AVG on the wire: nothing divided on the host side
    assert D.stream_ordered_collectives()


def test_forced_dp_one_rank_gloo(monkeypatch):
    """ESS_DP_FORCE / force_dp: in a ONE-rank process group the data-parallel branches are taken (bench.py and the -m gpu tests run
    the RCCL side of the step that way on a single-GPU box); without the switch a one-rank group is a no-op as before."""
    import socket
    import torch.distributed as dist
    from ess_amd.training import distributed as D
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    dist.init_process_group('gloo', rank=0, world_size=1, init_method=f'tcp://127.0.0.1:{port}')
    try:
        seen = []
        orig = dist.all_reduce
        monkeypatch.setattr(dist, 'all_reduce', lambda t, *a, **k: (seen.append(t.numel()), orig(t, *a, **k))[1])
        red = D.GradAllReducer()
        g = torch.arange(6, dtype=torch.float32)
        D.force_dp(False)
        assert not D.dp_active()
        red.launch(g)
        red.wait()
        assert seen == []
        D.force_dp(True)
        assert D.dp_active() and D.world_size() == 1
        red.launch(g)
        red.wait()
        assert seen == [6] and torch.equal(g, torch.arange(6, dtype=torch.float32))  # mean over one rank
        sums, n = D.reduce_validation_sums({'x': torch.tensor(1.5)}, 3)
        assert n == 3.0 and float(sums['x']) == 1.5
    finally:
        D.force_dp(False)
        dist.destroy_process_group()


def _dp8_worker(rank, world, port, ret):
    """One of EIGHT ranks (BASELINE config 4's world size) over gloo on CPU: (1) GradAllReducer.arm over the REAL decoder's parameter
    list (models/style_networks.py SemSegE2VID: 37 conv weights + biases) -- bucket boundaries never separate a weight from its bias,
    the buckets tile the flat buffer exactly, the averaged gradient equals the mean over the ranks; (2) reduce_validation_sums with an
    EMPTY shard on one rank and a key only some ranks report; (3) broadcast_module from rank 0 with differing initial weights."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from types import SimpleNamespace
    from ess_amd import functional as Fn
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.training import distributed as D
    torch.manual_seed(100 + rank)
    dec = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat')
    w0 = next(dec.parameters()).detach().clone()
    D.broadcast_module(dec, 0)
    wb = next(dec.parameters()).detach().clone()
    params = [p for p in dec.parameters() if p.requires_grad]
    sizes = [p.numel() for p in params]
    total = sum(sizes)
    flat = torch.empty(total)
    off = 0
    for i, k in enumerate(sizes):  # rank r's "gradient" of parameter i: the constant (r + 1) * (i + 1)
        flat[off:off + k] = float((rank + 1) * (i + 1))
        off += k
    opt = SimpleNamespace(param_groups=[{'params': params}], flat_grad=flat)
    red = D.GradAllReducer()
    red.arm(opt, n_buckets=3)
    bk = red._armed['buckets']
    tiles = [(b['lo'], b['hi']) for b in bk]
    ok_tiling = tiles[0][0] == 0 and tiles[-1][1] == total and all(tiles[i][1] == tiles[i + 1][0] for i in range(len(tiles) - 1))
    # a boundary may only sit in front of a conv weight (4-D): never between a weight and its bias
    starts = {0}
    o = 0
    for p, k in zip(params, sizes):
        if p.dim() == 4:
            starts.add(o)
        o += k
    ok_bounds = all(lo in starts for lo, _ in tiles)
    fired = []
    for p in reversed(params):  # backward order; only conv weights report (their launch completes the bias too)
        if p.dim() == 4:
            Fn.GRAD_READY_HOOK(p)
        fired.append(len(red.pending))
    red.wait()
    mean_rank = sum(range(1, world + 1)) / world
    off, err = 0, 0.0
    for i, k in enumerate(sizes):
        err = max(err, (flat[off:off + k] - mean_rank * (i + 1)).abs().max().item())
        off += k
    # (2) validation sums: rank 3's shard is empty; 'only_some' is reported by the even ranks
    D.force_dp(False)
    losses = {}
    n = 0
    if rank != 3:
        losses = {'semseg_sensor_b_loss': torch.tensor(float(rank + 1))}
        if rank % 2 == 0:
            losses['only_some'] = torch.tensor(10.0)
        n = 2
    tot, n_tot = D.reduce_validation_sums(losses, n)
    exp_loss = float(sum(r + 1 for r in range(world) if r != 3))
    exp_some = 10.0 * sum(1 for r in range(world) if r % 2 == 0 and r != 3)
    ok_val = abs(float(tot['semseg_sensor_b_loss']) - exp_loss) < 1e-6 and abs(float(tot['only_some']) - exp_some) < 1e-6 and n_tot == 2.0 * (world - 1)
    out = torch.tensor([float(ok_tiling), float(ok_bounds), err, float(ok_val), float((wb - w0).abs().max() > 0 if rank else 1.0),
                        float(len(bk)), float(max(fired))])
    gathered = [torch.zeros_like(out) for _ in range(world)]
    dist.all_gather(gathered, out)
    wsum = [torch.zeros_like(wb.flatten()[:8]) for _ in range(world)]
    dist.all_gather(wsum, wb.flatten()[:8].contiguous())
    if rank == 0:
        ret.put(([t.tolist() for t in gathered], [t.tolist() for t in wsum]))
    dist.destroy_process_group()


def test_data_parallel_world8_gloo_buckets_validation_broadcast():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    import socket
    with socket.socket() as sk:  # a port that was free a moment ago, as test_forced_dp_one_rank_gloo takes its own
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    world = 8
    procs = [ctx.Process(target=_dp8_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, ws = q.get(timeout=300)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r, row in enumerate(res):
        ok_tiling, ok_bounds, err, ok_val, changed, n_b, max_fired = row
        assert ok_tiling == 1.0 and ok_bounds == 1.0, (r, row)
        assert err < 1e-5 and ok_val == 1.0, (r, row)
        assert changed == 1.0, (r, row)  # every non-zero rank's weights were replaced by rank 0's
        assert n_b == 3.0 and max_fired == 3.0, (r, row)  # all three buckets were issued from inside the (simulated) backward
    assert all(w == ws[0] for w in ws)


def test_derived_weight_store_contract():
    """functional.derived: one store, one validity rule for every tensor derived from a weight (CPU tensors, a counting build)."""
    import gc

    from ess_amd import functional as Fn
    w, b = torch.randn(4, 6, 3, 3), torch.randn(4)
    builds = []

    def get(sources, key='k'):
        return Fn.derived(sources, key, lambda: builds.append(key) or torch.zeros(1))
    # an in-place op (_version) and a replaced .data (data_ptr) rebuild the entry
    v = get((w,))
    assert get((w,)) is v and len(builds) == 1
    w.mul_(1.0)
    assert get((w,)) is not v and len(builds) == 2
    w.data = w.data.clone()
    get((w,))
    get((w,))
    assert len(builds) == 3
    # invalidate: of the root, and of a non-root source only
    get((w, b), 'wb')
    assert len(builds) == 4
    Fn.invalidate([w])
    get((w,))
    get((w, b), 'wb')
    assert len(builds) == 6
    Fn.invalidate([b])
    get((w,))
    assert len(builds) == 6
    get((w, b), 'wb')
    assert len(builds) == 7
    # a derivation chain is filed under its root: dropping the root's entries drops the packs of its copies
    cols = Fn.columns(w, [(0, 2), (0, 2)])
    assert torch.equal(cols, torch.cat([w[:, :2], w[:, :2]], 1)) and Fn.columns(w, [(0, 2), (0, 2)]) is cols
    first = Fn.columns(w, [(0, 2)])
    assert torch.equal(first, w[:, :2])
    get((cols,), 'pack')
    get((first,), 'pack')
    get((cols,), 'pack')
    assert len(builds) == 9
    ents = Fn._entries(w)
    assert ents[(('cols', ((0, 2), (0, 2))), 'pack')].transform == Fn.REPEATED_COLUMNS
    assert ents[(('cols', ((0, 2),)), 'pack')].transform == Fn.FIRST_COLUMNS
    Fn.invalidate([w])
    assert Fn._entries(w) is None
    get((Fn.columns(w, [(0, 2), (0, 2)]),), 'pack')
    assert len(builds) == 10
    # snapshot / drop_unowned: owned keys survive (their entries stay valid), everything else under the parameter is dropped
    get((w,))
    snap = Fn.snapshot([w])
    assert all(k in snap[0][id(w)] for k in Fn._entries(w))
    owned = get((w,))
    get((w,), 'eager')
    get((Fn.columns(w, [(0, 3)]),), 'pack')
    n = len(builds)
    Fn.drop_unowned([w], snap)
    assert get((w,)) is owned and len(builds) == n
    assert ('eager' not in Fn._entries(w)) and (('cols', ((0, 3),)), 'pack') not in Fn._entries(w)
    get((w,), 'eager')
    assert len(builds) == n + 1
    # refresh keeps no pack of a column copy (nothing here is a layout the multi-tensor launch re-packs: no launch)
    get((Fn.columns(w, [(0, 3)]),), 'pack')
    Fn.refresh([w])
    assert Fn._entries(w) == {}
    # entries die with their root
    del snap, owned, v, cols, first
    rid = id(w)
    del w
    gc.collect()
    assert rid not in Fn._store
