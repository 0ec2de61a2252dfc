"""GPU: bench.py prints ONE JSON line with the contract's keys (small grid, a few steps): the single-GPU --full line with
`roofline`, `cpu_baseline` and `parity_rel_linf`, the plain lines without what only --full adds, the rehearsal lines of both
scaling modes marked as rehearsals, the cylindrical and the curved-solid variants."""
import json
import os
import subprocess
import sys

import pytest

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
        'dtype', 'data', 'config', 'roofline']


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]                   # exactly one line on stdout
    d = json.loads(lines[0])
    for k in KEYS:
        assert k in d, k
    assert d['higher_is_better'] is True and d['dtype'] == 'f64' and d['data'] == 'synthetic' and d['vs_baseline'] is None
    rf = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in rf, k
    assert rf['bound'] == 'hbm' and rf['peak'] == 8000.0 and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-3
    assert d['value'] > 0 and d['ms_per_step'] > 0 and 'workload' in d['config'] and 'model' not in d['config']
    return d


def test_single_gpu_line_with_cpu_baseline_and_parity():
    d = _bench('--n', '64', '--cpu-n', '64', '--steps', '4', '--warmup', '2', '--full')
    assert d['n_gpus'] == 1 and d['steps'] == 4 and d['warmup'] == 2 and d['scaling'] == 'weak'
    cb = d['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in cb, k
    assert cb['kind'] == 'port' and cb['cores'] == 1 and d['cpu_baseline_all_cores']['cores'] >= 1
    assert d['parity_rel_linf'] <= 1e-10 and d['parity']['steps'] == 3
    assert 'north_star_x_sweep' in d and d['north_star_x_sweep']['target_frac'] == 0.60
    assert 'prewarm' in d and set(d['general_pack_sweeps_42B']) == {'sweep_axis0', 'sweep_axis1', 'sweep_axis2_contig'}
    # the other BASELINE.json configurations ride in the same line (after the timed region)
    al = d['also']
    assert set(al) == {'config2_256', 'config4_cyl', 'ellipsoid_64', 'robin_field_ellipsoid_64'}
    for k, v in al.items():
        assert v['ms_per_step'] > 0 and v['steps_per_s'] > 0 and len(v['kernels']) >= 3, k
        for kk in v['kernels'].values():
            assert kk['ms'] > 0 and kk['bytes_per_cell'] >= 16 and 0 < kk['frac'] < 1, (k, kk)
    assert al['config4_cyl']['roofline']['bound'] == 'hbm' and set(al['config4_cyl']['kernels']) == {'sweep_r', 'sweep_phi', 'sweep_z_contig'}
    rf = al['robin_field_ellipsoid_64']
    assert rf['bytes_per_cell_step'] > al['ellipsoid_64']['bytes_per_cell_step']      # its sweeps load coefficient arrays
    assert rf['target_vs_scalar_h'] == 1.10 and rf['vs_scalar_h_ellipsoid'] > 0


def test_plain_lines_leave_the_extras_to_full():
    """without --full the line carries the headline and its per-stage figures, and nothing that takes runs of its own"""
    full_only = {'cpu_baseline', 'cpu_baseline_all_cores', 'parity', 'parity_rel_linf', 'also', 'general_pack_sweeps_42B',
                 'north_star_x_sweep', 'parity_vs_one_domain'}
    d = _bench('--n', '64', '--cpu-n', '64', '--steps', '4', '--warmup', '2')
    assert d['steps'] == 4 and d['warmup'] == 2 and 'prewarm' in d and len(d['kernels']) >= 3
    assert not full_only & set(d), sorted(full_only & set(d))
    d = _bench('--config', 'cyl', '--steps', '2', '--warmup', '1')
    assert d['metric'].startswith('adi_cyl') and not full_only & set(d), sorted(full_only & set(d))
    d = _bench('--n', '128', '--steps', '3', '--warmup', '2', '--force-dist')
    assert d['ranks']['backend'] == 'nccl' and not full_only & set(d), sorted(full_only & set(d))


@pytest.mark.parametrize('scaling,form', [('weak', 'deferred_exact'), ('strong', 'deferred_exact')])   # (256 rows at cfl 200: no decay)
def test_rehearsal_lines_are_marked(scaling, form):
    d = _bench('--n', '256', '--steps', '3', '--warmup', '2', '--no-cpu', '--rehearse-world', '4', '--scaling', scaling)
    assert 'rehearsal' in d and d['n_gpus'] == 1 and d['scaling'] == scaling
    assert d['comm_overlap']['axis0_interface'] == form and d['comm_overlap']['selfcheck_rel_diff'] <= 1e-12
    assert d['config']['planes_per_gpu'] == (256 if scaling == 'weak' else 64)


def test_curved_solid_and_cylindrical_lines():
    d = _bench('--n', '128', '--steps', '3', '--warmup', '2', '--no-cpu', '--mask', 'ellipsoid')
    assert 'ellipsoid' in d['config']['workload']
    d = _bench('--config', 'cyl', '--steps', '4', '--warmup', '2', '--no-cpu')
    assert d['metric'].startswith('adi_cyl') and set(d['kernels']) == {'sweep_r', 'sweep_phi', 'sweep_z_contig'}


@pytest.mark.parametrize('scaling', ['weak', 'strong'])
def test_two_real_ranks_line_proves_itself_against_one_domain(scaling):
    """`bench.py --gpus 2` started plainly: the parent starts two ranks (separate processes), here on the one GPU of the box
    over the gloo-staged test transport.  The line of an N > 1 run must carry `parity_vs_one_domain` -- 3 steps of the n^3 grid
    cut over the ranks against the same steps on one domain, <= 1e-12 -- and, with weak scaling, the
    same for the timed job's own slab thickness; plus the `ranks` record."""
    d = _bench('--gpus', '2', '--n', '128', '--steps', '3', '--warmup', '2', '--no-cpu', '--transport', 'gloo-staged',
               '--scaling', scaling, '--full')
    assert d['n_gpus'] == 2 and d['scaling'] == scaling
    p = d['parity_vs_one_domain']
    assert p['ok'] is True and p['rel_linf'] <= 1e-12 and p['bar'] == 1e-12 and p['steps'] == 3 and p['forms_agree']
    assert p['grid'] == '128x128x128' and p['planes_per_rank'] == [64, 64] and p['form'] is not None
    if scaling == 'weak':
        w = p['weak_form']
        assert w['ok'] is True and w['rel_linf'] <= 1e-12 and w['planes_per_rank'] == [128, 128] and w['grid'] == '256x128x128'
    else:
        assert 'weak_form' not in p
    r = d['ranks']
    assert r['world_size_from_process_group'] == 2 and 'gloo-staged' in r['transport'] and len(r['loop_seconds_per_rank']) == 2
    assert d['comm_overlap']['selfcheck_rel_diff'] <= 1e-12


def test_single_rank_rccl_line_runs_the_parity_calls_over_nccl():
    """--force-dist: the slab path over a one-rank RCCL process group; the calls of parity_vs_one_domain (gather, object
    all-gather, the one-domain leg) go through the real `nccl` backend here, the only place a one-GPU box can exercise them"""
    d = _bench('--n', '128', '--steps', '3', '--warmup', '2', '--no-cpu', '--force-dist', '--full')
    p = d['parity_vs_one_domain']
    assert p['ok'] is True and p['rel_linf'] <= 1e-12 and p['planes_per_rank'] == [128]
    assert d['ranks']['backend'] == 'nccl' and d['ranks']['world_size_from_process_group'] == 1


def test_dump_outputs_is_the_field_of_the_last_timed_step(tmp_path):
    """--dump-outputs: at 64^3 the whole field fits the budget, so T.npy is the field after warmup + steps steps from the seeded T0,
    checked against the single-thread oracle taking the same steps; the 128 MB cylindrical field goes out as a seeded sample plus
    its middle plane, all files fp64 and within the cap together"""
    import numpy as np
    d = _bench('--n', '64', '--steps', '3', '--warmup', '2', '--no-cpu', '--no-also', '--dump-outputs', str(tmp_path / 'cart'))
    assert d['steps'] == 3 and d['dumped_outputs'] == ['T.npy']
    got = np.load(str(tmp_path / 'cart' / 'T.npy'))
    assert got.dtype == np.float64 and got.shape == (64, 64, 64)
    sys.path.insert(0, ROOT)
    from oracle import adi_oracle as orc
    grid = orc.Grid3D(64, 64, 64, 5e-4, np.ones((64, 64, 64), bool))
    mat = orc.Material(7800.0, 490.0, 54.0)
    prm = orc.Params(200.0 * grid.dx ** 2 / (mat.k / (mat.rho * mat.cp)), 0.5)
    packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h=500.0)
    T0 = np.random.default_rng(1).uniform(20.0, 1000.0, (64, 64, 64))
    want = orc.adi_run(T0, grid, mat, prm, packs, Tinf=20.0, nsteps=5)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()

    d = _bench('--config', 'cyl', '--steps', '2', '--warmup', '1', '--no-cpu', '--dump-outputs', str(tmp_path / 'cyl'))
    assert d['dumped_outputs'] == ['T_mid_plane.npy', 'T_sample.npy']
    files = [str(tmp_path / 'cyl' / f) for f in d['dumped_outputs']]
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_BUDGET
    plane, sample = (np.load(f) for f in files)
    assert plane.dtype == sample.dtype == np.float64 and plane.shape == (256, 512) and sample.size == bench.DUMP_SAMPLE
    assert np.isfinite(sample).all() and 19.999 <= sample.min() and sample.max() <= 1000.001     # BE from T0 in [20, 1000]
    # the sampled cells are the ones dump_sample_cells names: those in plane nr // 2 equal the dumped middle plane
    i, j, k = np.unravel_index(bench.dump_sample_cells(128 * 256 * 512, sample.size), (128, 256, 512))
    mid = i == 64
    assert mid.sum() > 1000 and np.array_equal(sample[mid], plane[j[mid], k[mid]])
    T0 = np.full((128, 256, 512), 20.0); T0[:, :, -16:] = 1000.0
    assert np.any(sample != T0[i, j, k])                                                       # stepped, not the initial field


def test_dump_outputs_of_two_ranks_are_all_listed(tmp_path):
    """--gpus 2 (two real processes on the one GPU, gloo-staged test transport): each rank writes its own files in its half of the
    budget and the line lists the files of both ranks -- whole slabs (128^3 each) and sampled cylindrical replicas, which, started
    from the same field, are identical"""
    import numpy as np
    d = _bench('--gpus', '2', '--n', '128', '--steps', '2', '--warmup', '1', '--no-cpu', '--transport', 'gloo-staged',
               '--dump-outputs', str(tmp_path / 'cart'))
    assert d['dumped_outputs'] == ['T_rank0.npy', 'T_rank1.npy'] == sorted(os.listdir(str(tmp_path / 'cart')))
    for f in d['dumped_outputs']:
        a = np.load(str(tmp_path / 'cart' / f))
        assert a.dtype == np.float64 and a.shape == (128, 128, 128) and np.isfinite(a).all()
    d = _bench('--config', 'cyl', '--gpus', '2', '--steps', '2', '--warmup', '1', '--no-cpu', '--transport', 'gloo-staged',
               '--dump-outputs', str(tmp_path / 'cyl'))
    names = ['T_rank%d_%s.npy' % (r, w) for r in (0, 1) for w in ('mid_plane', 'sample')]
    assert d['dumped_outputs'] == names == sorted(os.listdir(str(tmp_path / 'cyl')))
    assert sum(os.path.getsize(str(tmp_path / 'cyl' / f)) for f in names) <= bench.DUMP_BUDGET
    for w in ('mid_plane', 'sample'):
        assert np.array_equal(np.load(str(tmp_path / 'cyl' / ('T_rank0_%s.npy' % w))),
                              np.load(str(tmp_path / 'cyl' / ('T_rank1_%s.npy' % w))))


def test_cylindrical_replicas_line():
    """`bench.py --config cyl --gpus 2`: the cylindrical path does not shard -- N independent replicas, the
    barrier and max-over-ranks timing of the contract; two real processes on the one GPU over the gloo-staged test transport"""
    d = _bench('--config', 'cyl', '--gpus', '2', '--steps', '4', '--warmup', '2', '--no-cpu', '--transport', 'gloo-staged')
    assert d['n_gpus'] == 2 and d['config']['decomposition'] == 'replicas only' and d['metric'].startswith('adi_cyl')
