#!/usr/bin/env python3
"""Generate tests/golden/eval_script_outputs.json with the REFERENCE's own evaluation scripts.

Runs only in the build container (needs the reference tree). Writes the run directories tests/test_evaluation.py
builds (`_write_run`: the two sequences of eval_sequence.txt / eval_sequence_b.txt, a scenario.yaml with the method
filled in), runs the reference's scripts/evaluation.py on them -- single-run mode on run0, multi-run mode on the base
directory -- and its scripts/paper/kitti_{odometry,artificial}_table.py, all importing `deepclr` from this
repository, and records what they left: the text of every CSV file, the relative path and size of every other file,
and the paper tables' stdout. tests/test_evaluation.py checks this package against that record without the scripts.

Usage:  python tests/golden/make_eval_script_golden.py  --reference <path of the reference tree>
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _files(base):
    out = {}
    for root, _, names in os.walk(base):
        for name in names:
            path = os.path.join(root, name)
            out[os.path.relpath(path, base)] = path
    return out


def _run(argv, cwd):
    done = subprocess.run([sys.executable] + argv, env=dict(os.environ, PYTHONPATH=REPO, MPLBACKEND='Agg'), cwd=cwd,
                          capture_output=True, text=True, timeout=600)
    if done.returncode != 0:
        raise SystemExit('{} failed:\n{}'.format(' '.join(argv), done.stderr[-3000:]))
    return done.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    scripts = os.path.join(os.path.abspath(args.reference), 'scripts')
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    sys.path.insert(0, REPO)
    from test_evaluation import _write_run
    record = {'evaluation': {}, 'paper': {}}
    with tempfile.TemporaryDirectory() as base:
        before = set(_files(base))
        _write_run(base, 'run0', 'DEEPCLR')
        _write_run(base, 'run1', 'DEEPCLR', sequential=False)
        inputs = set(_files(base))
        _run([os.path.join(scripts, 'evaluation.py'), os.path.join(base, 'run0')], base)
        _run([os.path.join(scripts, 'evaluation.py'), base, '--scenario', 'demo'], base)
        files = _files(base)
        rec = record['evaluation']
        rec['csv'] = {rel: open(p).read() for rel, p in sorted(files.items()) if rel.endswith('.csv')}
        rec['other_files'] = {rel: os.path.getsize(p) for rel, p in sorted(files.items())
                              if rel not in inputs and rel not in before and not rel.endswith('.csv')}
    for script, scenario in (('kitti_odometry_table.py', 'kitti_04_10'), ('kitti_artificial_table.py', 'kitti_pairs')):
        with tempfile.TemporaryDirectory() as base:
            _write_run(base, 'run0', 'DEEPCLR', scenario=scenario)
            record['paper'][script] = _run([os.path.join(scripts, 'paper', script), base], base)
    with open(os.path.join(HERE, 'eval_script_outputs.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
