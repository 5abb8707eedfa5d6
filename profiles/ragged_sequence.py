#!/usr/bin/env python3
"""Sequential odometry on frames of different sizes: pairs/s of ModelInferenceHelper.predict_sequence on a list of frames
(one sampler and one set-abstraction launch per size class) against the same chunk sizes as equal-size tensors at the class
maximum and against the per-frame predict loop (run on the GPU box, from the repo root):

    python3 profiles/ragged_sequence.py [--frames 128] [--reps 3]

Frames are LiDAR ring scans (deepclr_amd/synthetic.py:ring_scan) cut to N points, N drawn uniformly from [48000, 65536]
with a fixed seed: the density and the spread of frame sizes of KITTI odometry after the reference converter keeps every
second point. The KITTI architecture with random weights. Prints one JSON line:
  ragged[T]  predict_sequence(list of T frames), state carried from call to call (T pairs per call)
  equal[T]   predict_sequence((T, 65536, 4) tensor): the same kernels at the class maximum
  per_frame  predict(frame) once per frame (one sampler workgroup per launch)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepclr_amd import synthetic  # noqa: E402
from deepclr_amd.config import model_config_from_dict  # noqa: E402
from deepclr_amd.models import build_model, ModelInferenceHelper  # noqa: E402

N_LO, N_HI = 48000, 65536


def frames(count: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(N_LO, N_HI + 1, size=count)
    out = []
    for i, n in enumerate(sizes):
        scan = synthetic.ring_scan(np.random.default_rng(seed * 100003 + i), (int(n) + 31) // 32 * 32)[:n]
        out.append(torch.from_numpy(scan.astype(np.float32)))
    return out


def pad_to_class_max(f: torch.Tensor) -> torch.Tensor:
    """A frame at the class maximum: the frame's points, then its first points again (65536 in all)."""
    reps = (N_HI + f.shape[0] - 1) // f.shape[0]
    return f.repeat(reps, 1)[:N_HI]


def rate(run, chunks, pairs_per_call: int, reps: int) -> float:
    """pairs/s of run(chunk) over reps passes through the chunks, after one untimed warm-up call."""
    run(chunks[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for c in chunks:
            run(c)
    torch.cuda.synchronize()
    return reps * len(chunks) * pairs_per_call / (time.perf_counter() - t0)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=128, help='frames in the pool (a multiple of 128)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--loop-frames', type=int, default=64, help='frames the per-frame predict loop times')
    args = ap.parse_args()
    dev = 'cuda:0'
    cfg = synthetic.model_cfg('kitti')
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(synthetic.random_state_dict(cfg, seed=0))
    model = model.to(dev).eval()
    pool = [f.to(dev) for f in frames(args.frames)]
    out = {'metric': 'ragged_sequence_pairs_per_s', 'frames': args.frames, 'n_range': [N_LO, N_HI],
           'mean_n': float(np.mean([f.shape[0] for f in pool])), 'ragged': {}, 'equal': {}}
    for t in (64, 128):
        chunks = [pool[i:i + t] for i in range(0, len(pool), t)]
        seq = ModelInferenceHelper(model, is_sequential=True)
        seq.predict_sequence(chunks[0][:2])                                # a carried frame: every call yields t pairs
        out['ragged'][str(t)] = rate(seq.predict_sequence, chunks, t, args.reps)
        equal = [torch.stack([pad_to_class_max(f) for f in c]) for c in chunks]
        seq = ModelInferenceHelper(model, is_sequential=True)
        seq.predict_sequence(equal[0][:2])
        out['equal'][str(t)] = rate(seq.predict_sequence, equal, t, args.reps)
        del equal
        out.setdefault('ragged_over_equal', {})[str(t)] = out['ragged'][str(t)] / out['equal'][str(t)]
    loop = ModelInferenceHelper(model, is_sequential=True)
    loop.predict(pool[0])

    def per_frame(chunk):
        for f in chunk:
            loop.predict(f)
        loop.finish()
    k = args.loop_frames
    out['per_frame'] = rate(per_frame, [pool[1:1 + k]], k, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
