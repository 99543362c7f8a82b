#!/usr/bin/env python
"""Does a stream's result depend on the batch it rides in?  MultiStreamSegmenter at S = 8 against S = 1 on stream 3's grids, eager
and as a graph replay (2 x 480 x 640, K = 11, 'mixed', the encoder's space-to-depth form pinned), three windows: per pair of runs and
window (labels equal?, differing labels, max |confidence difference|).  --pin-norm-split also pins the slice count of the split
InstanceNorm statistics (hip.tuning_set('norm_split_wgs', hip.NORM_SPLIT_BY_PLANE)); --layers compares, for the first window and in
eager mode, every decoder stage's output of stream 3 with the solo run's, bit for bit, in the forms the next stage reads.
usage: python tools/batch_independence_probe.py [--pin-norm-split] [--layers] [--compute mixed]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--compute', default='mixed')
    ap.add_argument('--pin-norm-split', action='store_true')
    ap.add_argument('--layers', action='store_true')
    a = ap.parse_args()
    from oracle import ess_oracle as O
    from ess_amd import copies, hip
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.run_segmentation import MultiStreamSegmenter
    S, C, H, W, K, row = 8, 2, 480, 640, 11, 3
    cfg = O.e2vid_config(num_bins=C)
    sd_e = O.synth_state_dict(O.e2vid_param_shapes(cfg), 31)
    sd_d = O.synth_state_dict(O.semseg_param_shapes(256, K), 32, decoder_style=True)
    g = torch.Generator().manual_seed(77)
    grids = (torch.randn(3, S, C, H, W, generator=g) * (torch.rand(3, S, C, H, W, generator=g) < 0.2)).cuda()
    hip.set_compute(a.compute)
    set_s2d_mode('2')
    if a.pin_norm_split:
        hip.tuning_set('norm_split_wgs', hip.NORM_SPLIT_BY_PLANE)

    def models():
        m = E2VIDRecurrent(dict(cfg))
        m.load_state_dict(sd_e)
        d = SemSegE2VID(256, K, skip_connect=True, skip_type='concat')
        d.load_state_dict(sd_d)
        return m.cuda().eval(), d.cuda().eval()

    def forms(t):
        out = {}
        if torch.is_tensor(t):
            r = copies.of(t)
            if not r.unwritten and any(t.stride()):
                out['self'] = t
            if r.c8 is not None:
                out['c8'] = r.c8
            if r.h16 is not None:
                out['h16'] = r.h16[0]
        return out

    def run(n, graph, spy=None):
        enc, dec = models()
        r0 = row if n == S else 0
        if spy is not None:
            for nm, m in dec.named_modules():
                if nm.count('.') == 1 and nm.startswith('decoder_scale'):
                    m.register_forward_hook((lambda nm: lambda mod, i, o: spy.append((nm, {k: v[r0].clone() for k, v in forms(o).items()})))(nm))
                    if hasattr(m, 'forward_fused'):
                        m.forward_fused = (lambda ff, nm: lambda *aa, **kk: (lambda o: (spy.append((nm + '.fused', {k: v[r0].clone() for k, v in forms(o).items()})), o)[1])(ff(*aa, **kk)))(m.forward_fused, nm)
        seg = MultiStreamSegmenter(enc, dec, H, W, default_options(), n, graph=graph, want_confidence=True)
        out = []
        for w in range(1 if spy is not None else 3):
            r = seg.update(grids[w] if n == S else grids[w][row:row + 1])
            out.append((r.labels[r0].clone(), r.confidence[r0].clone()))
            if spy is not None:
                spy[:0] = [('latent%d' % k, {kk: v[r0].clone() for kk, v in forms(seg.last_latent[k]).items()}) for k in (1, 2, 4, 8)]
        torch.cuda.synchronize()
        return out

    if a.layers:
        sa, sb = [], []
        run(S, False, sa)
        run(1, False, sb)
        for (na, fa), (nb, fb) in zip(sa, sb):
            for k in fa:
                x, y = fa[k], fb[k]
                print(f'{na:28s} {k:8s} {str(x.dtype):15s} {tuple(x.shape)} equal={torch.equal(x.view(torch.uint8), y.view(torch.uint8))} '
                      f'max|d|={(x.float() - y.float()).abs().max().item():.3e}')
    else:
        res = {k: run(S if k[1] == '8' else 1, k[0] == 'g') for k in ('e8', 'g8', 'e1', 'g1')}
        ks = list(res)
        for i in range(len(ks)):
            for j in range(i + 1, len(ks)):
                print(ks[i], ks[j], [(bool(torch.equal(x[0], y[0])), int((x[0] != y[0]).sum()), float((x[1] - y[1]).abs().max()))
                                     for x, y in zip(res[ks[i]], res[ks[j]])])
    hip.set_compute('fp32')


if __name__ == '__main__':
    main()
