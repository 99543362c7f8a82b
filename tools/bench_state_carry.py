#!/usr/bin/env python
"""The masked state carry (hip.state_carry_masked) alone, at the state of S streams of a full-size segmenter, against the sequence
of whole-batch copy_ calls it replaces (GraphedWindowState._adopt_state: one per state tensor).

Run it under a kernel trace of its own -- no counters, no other tracing in that run --

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_state_carry.py --streams 8

and hand the trace to the same script:  python tools/bench_state_carry.py --parse <dir>/**/*_kernel_trace.csv
-> per case (all-TAKE, all-HOLD, half TAKE, the indexed gather of the same half, the copy_ sequence) the median time of one carry, the bytes it moves (read + written)
and the achieved TB/s.  The run itself also prints device-event times per carry for every case (launch gaps included), which is
the comparison with the copy_ sequence where the runtime performs those copies without a kernel the trace lists.  The launches
are told apart by name and order: `--reps` carries per case, the cases in the order above, a marker launch (a 1-element fill_ of
an int64 tensor) between them.  indexed_half is hip.state_carry_indexed gathering the (S + 1) // 2 even records of the S-stream
state into a batch of that size: the bytes of half_take through the indexed kernel, in the same trace run.  The run is one
process and stops at its first error; a wrapper that runs further steps behind it chains them on its exit status."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ('all_take', 'all_hold', 'half_take', 'indexed_half', 'copy_sequence')
KERNEL = {'indexed_half': 'state_carry_indexed'}  # (every other kernel case: state_carry_masked)


def run(a):
    import torch
    from ess_amd import hip
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.run_segmentation import MultiStreamSegmenter
    cfg = dict(num_bins=a.bins, skip_type='sum', num_encoders=3, base_num_channels=32, num_residual_blocks=2, norm='BN',
               use_upsample_conv=True, recurrent_block_type=a.recurrent)
    hip.set_compute(a.compute)
    torch.manual_seed(6)
    S = a.streams
    seg = MultiStreamSegmenter(E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat'), a.height,
                               a.width, default_options(), S)
    dst = seg._dst
    src = [torch.randn(t.shape, device=t.device).to(t.dtype) for t in dst]
    table = hip.StateCarryTable(dst, src)
    per_stream = sum(table.bytes_per_sample)
    dev = dst[0].device
    half = list(range(0, S, 2))
    work = [torch.zeros((len(half),) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in dst]
    gather = hip.StateMoveTable(work, src)
    g_dst = torch.arange(len(half), dtype=torch.int32, device=dev)
    g_src = torch.tensor(half, dtype=torch.int32, device=dev)
    modes = {'all_take': [1] * S, 'all_hold': [0] * S, 'half_take': [1 if s % 2 == 0 else 0 for s in range(S)]}
    marker = torch.zeros(1, dtype=torch.int64, device=dev)
    event_us = {}
    for name in CASES:
        marker.fill_(1)
        m = torch.tensor(modes[name], dtype=torch.int32, device=dev) if name in modes else None
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            if name == 'indexed_half':
                gather.run(g_dst, g_src)
            elif m is None:
                for d, s in zip(dst, src):
                    d.copy_(s)
            else:
                table.run(m)
            ev[i + 1].record()
        torch.cuda.synchronize()
        gaps = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(a.reps)]
        # (device events on the stream: a gap holds one carry plus its launch gaps -- the copy_ sequence pays one gap per tensor)
        event_us[name] = {'median': round(statistics.median(gaps), 2), 'min': round(min(gaps), 2), 'max': round(max(gaps), 2)}
    moved = {'all_take': 2 * S * per_stream, 'all_hold': 0, 'half_take': 2 * ((S + 1) // 2) * per_stream,
             'indexed_half': 2 * len(half) * per_stream, 'copy_sequence': 2 * S * per_stream}
    print(json.dumps({'streams': S, 'compute': a.compute, 'recurrent': a.recurrent, 'tensors': len(dst), 'reps': a.reps,
                      'state_bytes_per_stream': per_stream, 'bytes_moved': moved, 'event_us_per_carry': event_us,
                      'event_TB_per_s': {k: round(moved[k] / (event_us[k]['median'] * 1e-6) / 1e12, 3) for k in CASES}}))


def parse(a):
    rows = list(csv.DictReader(open(a.parse)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    name_of = lambda r: r.get('Kernel_Name') or r.get('Name')  # noqa: E731
    # the benchmark section starts at the LAST len(CASES) marker launches; the marker is an int64 fill
    is_marker = [('fill' in name_of(r).lower() or 'FillFunctor' in name_of(r)) and 'long' in name_of(r) for r in rows]
    marks = [i for i, m in enumerate(is_marker) if m][-len(CASES):]
    if len(marks) != len(CASES):
        raise SystemExit(f'found {len(marks)} marker launches, expected {len(CASES)}')
    moved = json.loads(a.bytes_moved) if a.bytes_moved else {}
    out = {}
    for ci, name in enumerate(CASES):
        seg = rows[marks[ci] + 1:(marks[ci + 1] if ci + 1 < len(CASES) else len(rows))]
        if name == 'copy_sequence':
            k = [r for r in seg if 'state_carry_' not in name_of(r)]
            n = a.tensors
            us = [sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in k[i:i + n]) / 1e3 for i in range(0, len(k) - n + 1, n)]
            span = [(int(k[i + n - 1]['End_Timestamp']) - int(k[i]['Start_Timestamp'])) / 1e3 for i in range(0, len(k) - n + 1, n)]
        else:
            k = [r for r in seg if KERNEL.get(name, 'state_carry_masked') in name_of(r)]
            us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in k]
            span = us
        if not us:  # (same-dtype copy_ calls may run as runtime copies that a kernel trace does not list: see the run's event times)
            out[name] = {'launches': len(k)}
            continue
        med = statistics.median(us)
        out[name] = {'launches': len(k), 'median_us': round(med, 2), 'min_us': round(min(us), 2), 'max_us': round(max(us), 2),
                     'median_span_us': round(statistics.median(span), 2)}
        if name in moved:
            out[name]['bytes_moved'] = moved[name]
            out[name]['TB_per_s'] = round(moved[name] / (med * 1e-6) / 1e12, 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--bins', type=int, default=5)
    ap.add_argument('--classes', type=int, default=11)
    ap.add_argument('--streams', type=int, default=8)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--recurrent', default='convlstm')
    ap.add_argument('--compute', default='mixed')
    ap.add_argument('--parse', default=None, help='a rocprofv3 *_kernel_trace.csv of a run of this script')
    ap.add_argument('--tensors', type=int, default=0, help='(--parse) state tensors per carry = copy_ calls per sequence')
    ap.add_argument('--bytes-moved', default=None, help="(--parse) the run's bytes_moved JSON object")
    a = ap.parse_args()
    parse(a) if a.parse else run(a)


if __name__ == '__main__':
    main()
