"""Result-file format and odometry metrics against fixtures written by the reference's evaluation code
(tests/golden/make_eval_golden.py) and by its evaluation scripts (tests/golden/make_eval_script_golden.py)."""
import csv
import io
import json
import os

import numpy as np
import pytest

from deepclr_amd import evaluation as ev

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _expected():
    return np.load(os.path.join(GOLDEN, 'eval_expected.npz'))


def test_reads_reference_file_and_rewrites_it_identically(tmp_path):
    src = os.path.join(GOLDEN, 'eval_sequence.txt')
    seq = ev.Sequence.read(src)
    assert len(seq) == 700 and seq.table().shape == (700, 26)
    out = tmp_path / 'kitti_00.txt'
    seq.write(str(out))
    assert out.read_text() == open(src).read()                      # same numbers, same text formatting
    again = ev.Evaluator.read(str(tmp_path))
    assert again.has_sequence('kitti_00') and len(again.get_sequence('kitti_00')) == 700


def test_pose_chain_and_path_length_match_reference():
    want = _expected()
    seq = ev.Sequence.read(os.path.join(GOLDEN, 'eval_sequence.txt'))
    np.testing.assert_allclose(ev.chain_poses(seq.prediction), want['poses_pred'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ev.chain_poses(seq.ground_truth), want['poses_gt'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ev.travelled(seq.ground_truth), want['distances_gt'], rtol=0, atol=1e-9)


def test_step_and_segment_errors_match_reference():
    want = _expected()
    seq = ev.Sequence.read(os.path.join(GOLDEN, 'eval_sequence.txt'))
    step = ev.step_errors(seq)
    np.testing.assert_allclose(step['translation'], want['step_translation'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(step['rotation'], want['step_rotation'], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(step['translation_rmse'], want['step_translation_rmse'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(step['rotation_chordal'], want['step_rotation_chordal'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(step['time'], want['step_time'])
    seg = ev.segment_errors(seq)
    assert np.array_equal(seg['first_frame'], want['seg_first'])
    assert np.array_equal(seg['segment_length'], want['seg_length'])
    np.testing.assert_allclose(seg['speed'], want['seg_speed'], rtol=1e-12)
    np.testing.assert_allclose(seg['translation'], want['seg_translation'], rtol=1e-8, atol=1e-14)
    np.testing.assert_allclose(seg['rotation'], want['seg_rotation'], rtol=1e-6, atol=1e-12)


def test_evaluator_collects_sequences_and_skips_the_stateless_first_frame(tmp_path):
    e = ev.Evaluator()
    e.add_transforms('a', 0.0, None, np.eye(4), 1.0)                 # sequential mode: no prediction yet
    t = np.eye(4)
    t[0, 3] = 1.0
    for i in range(5):
        e.add_transforms('a', 0.1 * i, t, t, 2.0)
    e.add_transforms('b', 0.0, np.eye(4), t, 3.0)
    assert list(e.get_sequences()) == ['a', 'b'] and len(e.get_sequence('a')) == 5
    e.write(str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ['a.txt', 'b.txt']
    s = ev.Evaluator.read(str(tmp_path)).summary()
    assert abs(s['step_translation_mean [m]'] - 1.0 / 6) < 1e-12      # five exact pairs, one off by 1 m
    assert abs(s['time_mean [ms]'] - 13.0 / 6) < 1e-12
    assert np.isnan(s['kitti_translation [%]'])                      # 5 m driven: no 100 m segment exists


STATS = ('min', 'max', 'mean', 'median', 'std')
STEP_FIELDS = (('translation', 'kitti'), ('translation', 'rmse'), ('rotation', 'kitti'), ('rotation', 'chordal'))
SEG_FIELDS = STEP_FIELDS + (('rotation', 'rmse'),)


def _two_sequences():
    e = ev.Evaluator()
    e.get_sequences()['a'] = ev.Sequence.read(os.path.join(GOLDEN, 'eval_sequence.txt'))
    e.get_sequences()['b'] = ev.Sequence.read(os.path.join(GOLDEN, 'eval_sequence_b.txt'))
    return e


def test_metrics_container_statistics_match_reference():
    """min / max / mean / median / std of every field scripts/evaluation.py:55-78 prints, per sequence and merged,
    against the reference's MetricsContainer (including the segment fields its `divide` derives from kitti)."""
    want = _expected()
    e = _two_sequences()
    groups = (('step', e.get_step_errors(), e.get_total_step_errors(), STEP_FIELDS),
              ('seg', e.get_segment_errors(), e.get_total_segment_errors(), SEG_FIELDS))
    for kind, per_seq, total, fields in groups:
        for name, cont in list(per_seq.items()) + [('total', total)]:
            assert len(cont) == int(want['{}_{}_count'.format(kind, name)])
            for stat in STATS:
                rec = getattr(cont, stat)
                got = [getattr(getattr(rec, part), metric) for part, metric in fields] + [rec.time]
                np.testing.assert_allclose(got, want['{}_{}_{}'.format(kind, name, stat)], rtol=2e-6, atol=1e-13,
                                           err_msg='{} {} {}'.format(kind, name, stat))
    assert e.get_total_step_errors() is e.get_total_step_errors()            # cached until transforms are added
    e.add_transforms('b', 0.0, np.eye(4), np.eye(4), 1.0)
    assert len(e.get_total_step_errors()) == 700 + 260 + 1


def test_metrics_container_items_and_empty_case():
    e = _two_sequences()
    seg = e.get_segment_errors()['b']
    item = seg[3]
    assert item.segment_length == seg.arrays['segment_length'][3] and item.first_frame == seg.arrays['first_frame'][3]
    assert item.translation.kitti == seg.arrays['translation'][3] and item.time == 0.0
    assert item.rotation.chordal == item.rotation.kitti / item.segment_length        # metrics.py:104-108
    assert [x.speed for x in seg] == list(seg.arrays['speed'])
    step = e.get_step_errors()['b']
    assert step[-1].time == step.arrays['time'][-1] and step.mean.translation.vec.shape == (3,)
    with np.testing.assert_raises(IndexError):
        step[len(step)]
    short = ev.Evaluator()
    t = np.eye(4)
    t[0, 3] = 1.0
    short.add_transforms('s', 0.0, t, t)
    empty = short.get_total_segment_errors()
    assert len(empty) == 0 and np.isnan(empty.mean.translation.kitti) and np.isnan(empty.max.rotation.vec).all()


def _euler_to_matrix(angles):
    out = []
    for rx, ry, rz in angles:
        cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
        mx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        my = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        mz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        out.append(mz @ my @ mx)
    return np.array(out)


def test_euler_angles_recompose_and_feed_the_rotation_rmse():
    """transforms3d is absent (parity unpinned for these fields): the static-xyz angles must rebuild the matrix they
    came from, also at the pitch singularity, and the per-pair rotation rmse is their rms difference."""
    rng = np.random.default_rng(5)
    angles = rng.uniform([-np.pi, -np.pi / 2, -np.pi], [np.pi, np.pi / 2, np.pi], size=(200, 3))
    np.testing.assert_allclose(ev.euler_sxyz(_euler_to_matrix(angles)), angles, rtol=0, atol=1e-12)
    gimbal = _euler_to_matrix(np.array([[0.3, np.pi / 2, -0.8], [-1.1, -np.pi / 2, 0.4]]))
    got = ev.euler_sxyz(gimbal)
    assert (got[:, 2] == 0).all()
    np.testing.assert_allclose(_euler_to_matrix(got), gimbal, rtol=0, atol=1e-12)
    a, b = np.tile(np.eye(4), (3, 1, 1)), np.tile(np.eye(4), (3, 1, 1))
    a[:, :3, :3] = _euler_to_matrix(np.array([[0.01, 0.02, 0.03], [0, 0, 0.5], [0.2, -0.1, 0.0]]))
    b[:, :3, :3] = _euler_to_matrix(np.array([[0.00, 0.02, 0.00], [0, 0, 0.1], [0.2, -0.1, 0.0]]))
    np.testing.assert_allclose(ev.euler_rmse(a, b), np.sqrt(np.array([0.01 ** 2 + 0.03 ** 2, 0.4 ** 2, 0.0]) / 3),
                               rtol=0, atol=1e-12)
    seq = ev.Sequence()
    for i in range(3):
        seq.add_transforms(i, a[i], b[i])
    err = ev.step_errors(seq)
    np.testing.assert_allclose(err['rotation_rmse'], ev.euler_rmse(a, b))
    # rotation-only error about z: the kitti angle is the yaw difference and its vector carries it on the z slot
    np.testing.assert_allclose(err['rotation'][1], 0.4, atol=1e-12)
    np.testing.assert_allclose(np.abs(err['rotation_vec'][1]), [0, 0, 0.4], atol=1e-12)


def test_motion_views_and_pose_export(tmp_path):
    seq = ev.Sequence.read(os.path.join(GOLDEN, 'eval_sequence_b.txt'))
    m = seq.prediction
    assert len(m) == 260 and m.poses.shape == (261, 4, 4) and m.get_path().shape == (261, 3)
    assert np.array_equal(m.poses[0], np.eye(4)) and m.distances[0] == 0
    f = m.get_frame_by_distance(10, 100)
    assert m.distances[f] > m.distances[10] + 100 >= m.distances[f - 1]
    assert m.get_frame_by_distance(10, 1e6) == -1
    m.write(str(tmp_path / 'poses.txt'), use_poses=True)                  # scripts/export_kitti_poses.py:28-33
    np.testing.assert_allclose(np.loadtxt(str(tmp_path / 'poses.txt')), m.poses[:, :3, :].reshape(-1, 12))


def _write_run(base, name, method, sequential=True, scenario='demo'):
    """A run directory as scripts/inference.py leaves it: result files + scenario.yaml with the method filled in."""
    import yaml
    d = os.path.join(base, name)
    os.makedirs(d)
    e = _two_sequences()
    e.write(d)
    with open(os.path.join(d, 'scenario.yaml'), 'w') as f:
        yaml.safe_dump({'name': scenario, 'dataset_type': 'GENERIC', 'sequential': sequential,
                        'data': {'a': '/data/a', 'b': '/data/b'},
                        'method': {'name': method, 'params': {'model_name': name, 'weights_file': 'w.tar'}}}, f)
    return d


def test_evaluation_flow_of_the_reference_script(tmp_path):
    """The call sequence of scripts/evaluation.py:83-140 on a run directory written by this build: scenario with
    method, step / segment tables via the `error.<stat>.<part>.<metric>` attributes, every figure saved."""
    import matplotlib
    matplotlib.use('Agg')
    from deepclr.evaluation import Evaluator, MetricsContainer, load_scenario
    want = _expected()
    d = _write_run(str(tmp_path), 'run0', 'DEEPCLR')
    scenario = load_scenario(os.path.join(d, 'scenario.yaml'), with_method=True)
    assert scenario.method.name == 'DEEPCLR' and scenario.method.params['model_name'] == 'run0'
    evaluator = Evaluator.read(d, ['{}.txt'.format(k) for k in scenario.data.keys()])
    total = evaluator.get_total_segment_errors()
    assert isinstance(total, MetricsContainer)
    np.testing.assert_allclose([total.mean.translation.kitti * 100, np.rad2deg(total.mean.rotation.kitti)],
                               [want['seg_total_mean'][0] * 100, np.rad2deg(want['seg_total_mean'][2])], rtol=2e-6)
    figures = [evaluator.plot_segment_error_bars(), evaluator.plot_total_kitti_errors()]
    for group in (evaluator.plot_error_over_time(), evaluator.plot_kitti_errors(), evaluator.plot_sequences(),
                  evaluator.plot_sequences_2d()):
        assert list(group) == ['a', 'b']
        figures.extend(group.values())
    for i, fig in enumerate(figures):
        out = tmp_path / 'fig{}.png'.format(i)
        fig.savefig(str(out), dpi=40)
        assert out.stat().st_size > 500
        matplotlib.pyplot.close(fig)
    from deepclr_amd import plots
    c = plots.kitti_curves(total)
    assert list(c['length']) == [100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0]
    a = total.arrays
    np.testing.assert_allclose(c['by_length'][2, 0], a['translation'][a['segment_length'] == 300].mean())
    counted = np.nansum([((a['speed'] > lo) & (a['speed'] <= hi)).sum() for lo, hi in
                         zip(np.linspace(a['speed'].min(), a['speed'].max(), 12)[:-1],
                             np.linspace(a['speed'].min(), a['speed'].max(), 12)[1:])])
    assert counted == len(total) - (a['speed'] == a['speed'].min()).sum()


def _script_record():
    """What the reference's scripts/evaluation.py and scripts/paper/kitti_*_table.py left on the run directories of
    `_write_run` (tests/golden/make_eval_script_golden.py): CSV texts, the other files by path, the tables' stdout."""
    with open(os.path.join(GOLDEN, 'eval_script_outputs.json')) as f:
        return json.load(f)


def _csv_rows(text):
    return list(csv.DictReader(io.StringIO(text)))


def _column_value(container, column):
    """The figure a column of the script's tables holds, read off this package's container: `<t|r>_<metric>_<stat>
    [unit]` is the `<stat>.<translation|rotation>.<metric>` attribute, `time_<stat> [ms]` is `<stat>.time`; angles are
    tabulated in degrees and a `%` column is the (per-metre) translation x 100."""
    name, unit = column[:-1].split(' [')
    if name.startswith('time_'):
        return getattr(container, name[len('time_'):]).time
    part, metric, stat = name.split('_')
    value = getattr(getattr(getattr(container, stat), {'t': 'translation', 'r': 'rotation'}[part]), metric)
    if unit.startswith('deg'):
        return np.rad2deg(value)
    return value * 100 if unit == '%' else value


def _check_rows(rows, containers):
    """Every numeric column of every row equals the figure this package's container for that row gives."""
    assert [r['name'] for r in rows] == list(containers)
    for row in rows:
        for column, text in row.items():
            if column in ('name', 'method', 'params'):
                continue
            np.testing.assert_allclose(_column_value(containers[row['name']], column), float(text), rtol=1e-9,
                                       atol=1e-15, err_msg='{} {}'.format(row['name'], column))


def _evaluate_run(d):
    from deepclr.evaluation import Evaluator, load_scenario
    scenario = load_scenario(os.path.join(d, 'scenario.yaml'), with_method=True)
    return scenario, Evaluator.read(d, ['{}.txt'.format(k) for k in scenario.data.keys()])


FIGURES = {'segment_errors': 'plot_segment_error_bars', 'plot_eot': 'plot_error_over_time',
           'plot_error': 'plot_kitti_errors', 'plot_path': 'plot_sequences', 'plot_path2d': 'plot_sequences_2d'}


def test_reference_evaluation_script_runs_on_this_builds_output(tmp_path):
    """f3 end to end: the reference's own scripts/evaluation.py, importing `deepclr` from this repository, evaluated
    run directories written here (single and multi-run mode; its outputs are stored in
    tests/golden/eval_script_outputs.json). Every figure of its CSV tables is read again off this package's containers
    through the attributes the script names in the column headers, the tables carry the golden statistics, and every
    figure file it saved is drawn again here."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    want = _expected()
    rec = _script_record()['evaluation']
    base = str(tmp_path)
    runs = {name: _evaluate_run(_write_run(base, name, 'DEEPCLR', sequential=name == 'run0')) for name in ('run0', 'run1')}
    scenario, evaluator = runs['run0']
    steps = dict(evaluator.get_step_errors(), TOTAL=evaluator.get_total_step_errors())
    _check_rows(_csv_rows(rec['csv']['run0/evaluation/step_errors.csv']), steps)
    rows = {r['name']: r for r in _csv_rows(rec['csv']['run0/evaluation/step_errors.csv'])}
    assert list(rows) == ['a', 'b', 'TOTAL']
    for name, key in (('a', 'step_a'), ('b', 'step_b'), ('TOTAL', 'step_total')):
        mean, std, mx = want[key + '_mean'], want[key + '_std'], want[key + '_max']
        got = rows[name]
        np.testing.assert_allclose(
            [float(got['t_kitti_mean [m]']), float(got['t_rmse_std [m]']), float(got['r_kitti_max [deg]']),
             float(got['r_chordal_mean [deg]']), float(got['time_mean [ms]']), float(got['time_max [ms]'])],
            [mean[0], std[1], np.rad2deg(mx[2]), np.rad2deg(mean[3]), mean[4], mx[4]], rtol=2e-6)
    segments = dict(evaluator.get_segment_errors(), TOTAL=evaluator.get_total_segment_errors())
    _check_rows(_csv_rows(rec['csv']['run0/evaluation/segment_errors.csv']), segments)
    rows = {r['name']: r for r in _csv_rows(rec['csv']['run0/evaluation/segment_errors.csv'])}
    mean, std = want['seg_total_mean'], want['seg_total_std']
    np.testing.assert_allclose(
        [float(rows['TOTAL']['t_kitti_mean [%]']), float(rows['TOTAL']['r_kitti_std [deg/m]']),
         float(rows['TOTAL']['r_rmse_mean [deg/m]'])],
        [mean[0] * 100, np.rad2deg(std[2]), np.rad2deg(mean[4])], rtol=2e-6)
    # every file the script saved (run0 only: run1 is not sequential and has no figures) is drawn again from this package
    assert not any(path.startswith('run1/') for path in rec['other_files'])
    for sub in ('segment_errors.png', 'plot_eot/a.pdf', 'plot_error/b.png', 'plot_path/a.png', 'plot_path2d/b.pdf'):
        assert rec['other_files']['run0/evaluation/' + sub] > 1000
    saved = {}                                                         # figure source -> {sequence or None: [paths]}
    for path in rec['other_files']:
        parts = path.split('/')
        assert parts[:2] == ['run0', 'evaluation'] and len(parts) in (3, 4), path
        source = os.path.splitext(parts[2])[0] if len(parts) == 3 else parts[2]
        key = None if len(parts) == 3 else os.path.splitext(parts[3])[0]
        saved.setdefault(source, {}).setdefault(key, []).append(path)
    for source, by_key in sorted(saved.items()):
        figs = getattr(evaluator, FIGURES[source])()
        if None not in by_key:
            assert list(figs) == ['a', 'b'] == sorted(by_key)
        for key, paths in by_key.items():
            fig = figs if key is None else figs[key]
            for path in paths:
                out = tmp_path / ('drawn_' + path.replace('/', '_'))
                fig.savefig(str(out), dpi=40)
                assert out.stat().st_size > 1000, path
        plt.close('all')
    # multi-run mode: one row per run directory of the scenario, method and parameters from its scenario.yaml
    rows = _csv_rows(rec['csv']['evaluation/demo/demo_step_errors.csv'])
    assert [r['name'] for r in rows] == ['run0', 'run1'] and rows[0]['method'] == 'DEEPCLR'
    assert 'model_name=run1' in rows[1]['params']
    for row in rows:
        scen = runs[row['name']][0]
        assert scen.name == 'demo' and row['method'] == scen.method.name
        assert all('{}={}'.format(k, v) in row['params'] for k, v in scen.method.params.items())
    _check_rows(rows, {name: ev_.get_total_step_errors() for name, (_, ev_) in runs.items()})
    rows = _csv_rows(rec['csv']['evaluation/demo/demo_segment_errors.csv'])
    assert len(rows) == 1 and scenario.sequential and not runs['run1'][0].sequential     # run1: not sequential
    _check_rows(rows, {'run0': evaluator.get_total_segment_errors()})
    _check_rows(_csv_rows(rec['csv']['run1/evaluation/step_errors.csv']),
                dict(runs['run1'][1].get_step_errors(), TOTAL=runs['run1'][1].get_total_step_errors()))


def _printed(texts, values):
    """Figures a pandas table printed (6 decimals at most) against the values they were printed from."""
    assert len(texts) == len(values)
    for text, value in zip(texts, values):
        assert abs(float(text) - value) <= 5e-7 * (1 + 1e-9), (text, value)


@pytest.mark.parametrize('script,scenario,expect', [
    ('kitti_odometry_table.py', 'kitti_04_10', ('t_rmse [m]', 'r_rmse [deg]', 'Average Inference Time')),
    ('kitti_artificial_table.py', 'kitti_pairs', ('Rot. Error Mean [deg]', 'Time [ms]')),
])
def test_reference_paper_tables_read_this_builds_output(tmp_path, script, scenario, expect):
    """scripts/paper/*_table.py (the tables of the publication) on a run directory written here (their stdout is
    stored in tests/golden/eval_script_outputs.json): they read `metrics.<stat>.<part>.<metric>` and `.time` off the
    containers, and the figures they printed are the ones this package's containers give."""
    stdout = _script_record()['paper'][script]
    for word in expect:
        assert word in stdout, stdout[-1500:]
    found, evaluator = _evaluate_run(_write_run(str(tmp_path), 'run0', 'DEEPCLR', scenario=scenario))
    assert found.name == scenario and found.method.name == 'DEEPCLR'
    total = evaluator.get_total_step_errors()
    want = _expected()
    if script == 'kitti_odometry_table.py':
        lines = stdout.splitlines()
        for seq, metrics in evaluator.get_step_errors().items():
            row = [l for l in lines if l.split()[:1] == [seq]]
            assert len(row) == 1, stdout
            _printed(row[0].split()[1:], [metrics.mean.translation.rmse, np.rad2deg(metrics.mean.rotation.rmse)])
        assert 'Average Inference Time: {:.2f} ms'.format(total.mean.time) in stdout
    if script == 'kitti_artificial_table.py':                 # one row of totals (pandas elides the middle columns at 80 characters)
        assert '{:.6f}'.format(np.rad2deg(want['step_total_mean'][3])) in stdout
        row = [l for l in stdout.splitlines() if l.startswith('DEEPCLR')]
        assert len(row) == 1 and row[0].split()[2] == '...'
        _printed(row[0].split()[1::2], [np.rad2deg(total.mean.rotation.chordal), total.mean.time])
