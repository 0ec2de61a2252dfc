"""Cases of tests/test_cyl_switches_gpu.py and tests/test_cyl_ref_cpu.py: one deterministic cylindrical case per dispatch
decision of csrc/adi_cyl.hip (cyl_sweep_r / phi / z, strided_rows, contig_rows) and csrc/adi_cyl_plan.hpp (cyl_pick_fast), and the
time-step sweep against the extended-precision reference tests/cyl_ref_ld.py.  Reference-free."""
import functools
import types
import zlib

import numpy as np

import cyl_ref_ld

STEEL = dict(rho=7800.0, cp=490.0, k=54.0)
ALPHA = STEEL['k'] / (STEEL['rho'] * STEEL['cp'])
DR = DZ = 2.5e-4
ROBIN_R = (400.0, 20.0)
ROBIN_INNER = (10.0, 45.0)
ROBIN_VOID = (5.0, 27.0)
NR_ROBIN = ('neumann0', 'robin')           # the reference drivers' closure pair
Z_OPEN_PAIRS = [('neumann0', 'neumann0'), ('neumann0', 'robin'), ('robin', 'neumann0'), ('robin', 'robin')]

# (kernel the case is meant to reach, (nr, nphi, nz), z closure pairs).  The other two sweeps of a case run whatever their
# extents select; DESIGN.md ("Cylindrical kernels: what reaches what") lists all three kernels of every case.
_P = [NR_ROBIN]
SWITCH_CASES = [
    # ---- r sweep
    ('r_fast16_2tiles', (256, 8, 16), _P),
    ('r_fast8_1tile', (64, 16, 4), _P),
    ('r_fast8_3tiles', (128, 8, 24), _P),
    ('r_strided8_fast_declined_plane45', (256, 5, 9), _P),      # tables present, plane % 64 != 0
    ('r_strided8_fast_declined_plane21', (64, 3, 7), _P),
    ('r_strided2_n16', (16, 3, 5), _P),
    ('r_strided4_n17', (17, 3, 5), _P),
    ('r_strided4_n32', (32, 3, 5), _P),
    ('r_strided8_n33', (33, 3, 5), _P),
    ('r_strided8_n512_8lines', (512, 3, 5), _P),                # Lp = 64: the LDS bound cuts the tile to 8 lines
    ('r_strided16_n513', (513, 3, 5), _P),
    ('r_strided16_n1024', (1024, 2, 9), _P),
    # ---- phi sweep
    ('phi_fast8_1tile', (3, 64, 32), _P),
    ('phi_fast8_3tiles', (3, 64, 96), _P),
    ('phi_fast16_Lp8', (3, 128, 32), _P),
    ('phi_fast16_Lp16', (2, 256, 64), _P),
    ('phi_fast16_Lp32', (2, 512, 32), _P),
    ('phi_strided8_fast_declined_nz48', (3, 128, 48), _P),      # nz % 32 != 0
    ('phi_strided8_fast_declined_n192', (3, 192, 32), _P),      # 12 segments of 16 / 24 of 8: not a power of two
    ('phi_strided8_fast_declined_n72', (3, 72, 32), _P),        # 9 segments of 8
    ('phi_strided2_n16', (3, 16, 8), _P),
    ('phi_strided4_n17', (3, 17, 8), _P),
    ('phi_strided8_n33', (3, 33, 8), _P),
    ('phi_strided16_n513', (2, 513, 8), _P),
    ('phi_strided16_n1024', (2, 1024, 8), _P),
    # ---- z sweep: k_cyl_z_fast<16> with 8 / 4 / 2 / 1 lines per wave, every closure pair it serves
    ('z_fast_lwf8', (3, 8, 128), Z_OPEN_PAIRS),
    ('z_fast_lwf4', (3, 4, 256), Z_OPEN_PAIRS),
    ('z_fast_lwf2', (3, 2, 512), Z_OPEN_PAIRS),
    ('z_fast_lwf1', (3, 3, 1024), Z_OPEN_PAIRS),
    # ---- z sweep: FAST declined by each of its conditions in turn
    ('z_contig2_fast_declined_nphi12', (3, 12, 128), _P),       # nphi % (64 / (nz / 16)) != 0
    ('z_contig4_fast_declined_nz144', (3, 8, 144), _P),         # 9 segments of 16
    ('z_contig2_fast_declined_dirichlet', (3, 8, 128), [('dirichlet', 'robin'), ('neumann0', 'dirichlet'),
                                                         ('dirichlet', 'dirichlet')]),
    # ---- z sweep: contig_rows 2 -> 4 -> 8 -> 16, the vector (VEC) and the scalar form
    ('z_contig2_vec_n128', (3, 5, 128), _P),
    ('z_contig4_scalar_n129', (3, 5, 129), _P),                 # nz % 4 != 0 (and an odd plane stride)
    ('z_contig4_vec_n256', (3, 5, 256), _P),
    ('z_contig8_scalar_n257', (3, 5, 257), _P),
    ('z_contig8_vec_n512', (3, 5, 512), _P),
    ('z_contig16_scalar_n513', (3, 5, 513), _P),
    ('z_contig16_scalar_n1000', (2, 3, 1000), _P),              # 1000 % 16 != 0
    ('z_fast_lwf1_nphi3', (2, 3, 1024), _P),                    # one line per wave divides any nphi: FAST, not contig<16>
    ('z_contig16_vec_n1024_dirichlet', (2, 3, 1024), [('dirichlet', 'robin')]),
    ('z_contig16_vec_n768', (2, 3, 768), _P),                   # 48 segments of 16: FAST declines
]

MODES = ('plain', 'source', 'masked')
R_INS = (0.0, 0.03)


def switch_params():
    """(id, case) for every entry x closure pair x inner radius x mode"""
    out = []
    for name, shape, pairs in SWITCH_CASES:
        for pair in pairs:
            for R_in in R_INS:
                for mode in MODES:
                    tag = '%s-%dx%dx%d-%s_%s-%s-%s' % ((name,) + shape + pair + ('axis' if R_in == 0.0 else 'annulus', mode))
                    out.append((tag, dict(shape=shape, pair=pair, R_in=R_in, mode=mode, dt=0.3)))
    return out


def make_case(shape, pair=NR_ROBIN, R_in=0.0, mode='plain', dt=0.3, nsteps=2):
    """the inputs of one case, drawn from a generator seeded by the case itself"""
    nr, nphi, nz = shape
    rng = np.random.default_rng(zlib.crc32(repr((shape, pair, R_in, mode)).encode()))
    c = dict(shape=shape, dr=DR, dz=DZ, dphi=2.0 * np.pi / nphi, R_in=float(R_in), mat=dict(STEEL), robin_r=ROBIN_R,
             zbc=dict(kind_bot=pair[0], kind_top=pair[1], h_bot=120.0, h_top=500.0, T_inf_bot=25.0, T_inf_top=15.0,
                      T_bot=300.0, T_top=80.0),
             dt=float(dt), nsteps=nsteps, T0=rng.uniform(20.0, 1200.0, shape), S=None, active=None, mode=mode)
    if mode == 'source':
        c['S'] = rng.uniform(0.0, 3e8, shape)
    elif mode == 'masked':
        c['active'] = rng.random(shape) > 0.3              # ~70 % fill: void and axis clamps live in the load and store paths
        c['robin_inner'] = ROBIN_INNER; c['robin_void'] = ROBIN_VOID
    return c


def api_objects(api, c):
    nr, nphi, nz = c['shape']
    grid = api.GridCyl(nr, nphi, nz, c['dr'], c['dphi'], c['dz'], c['R_in'] + nr * c['dr'], R_in=c['R_in'])
    return grid, api.Material(**c['mat']), api.Params(c['dt'], 1.0, "be"), api.RobinR(*c['robin_r']), api.ZBC(**c['zbc'])


def run_case(api, c):
    """c['nsteps'] steps through a module with the reference's operator surface (oracle.cyl_oracle, adi3d_hip_cyl)"""
    grid, mat, prm, rr, zbc = api_objects(api, c)
    T = np.array(c['T0'])
    for _ in range(c['nsteps']):
        if c['active'] is not None:
            T = api.adi_step_masked(T, grid, mat, prm, rr, zbc, c['active'], robin_inner=api.RobinR(*c['robin_inner']),
                                    robin_void=api.RobinR(*c['robin_void']))
        else:
            T = api.adi_step(T, grid, mat, prm, rr, zbc, S=c['S'])
    return np.asarray(T)


def run_ref_ld(c):
    """the same through tests/cyl_ref_ld.py, every step in np.longdouble; returns the longdouble field"""
    ns = types.SimpleNamespace
    nr, nphi, nz = c['shape']
    grid = ns(nr=nr, nphi=nphi, nz=nz, dr=c['dr'], dphi=c['dphi'], dz=c['dz'], R_in=c['R_in'])
    mat = ns(**c['mat']); prm = ns(dt=c['dt'])
    rr = ns(h=c['robin_r'][0], T_inf=c['robin_r'][1]); zbc = ns(**c['zbc'])
    T = np.asarray(c['T0'], dtype=np.longdouble)
    for _ in range(c['nsteps']):
        if c['active'] is not None:
            ri = ns(h=c['robin_inner'][0], T_inf=c['robin_inner'][1]); rv = ns(h=c['robin_void'][0], T_inf=c['robin_void'][1])
            T = cyl_ref_ld.adi_step_masked(T, grid, mat, prm, rr, zbc, c['active'], robin_inner=ri, robin_void=rv)
        else:
            T = cyl_ref_ld.adi_step(T, grid, mat, prm, rr, zbc, S=c['S'])
    return T


# ---- time-step range (section "Time step" of DESIGN.md's "Cylindrical kernels: what reaches what") -------------------
DT_SHAPES = [('r_fast16', (256, 8, 16)), ('r_fast8', (64, 16, 4)), ('phi_fast16_Lp32', (2, 512, 32)),
             ('phi_fast8', (3, 64, 32)), ('z_fast', (3, 2, 512)), ('general', (33, 17, 129))]
DT_F = [1e-13, 1e-9, 1e-3, 0.3, 3e4, 1e6]                   # alpha dt / dr^2
_PHI_SHAPES = ('phi_fast16_Lp32', 'phi_fast8')


def dt_params():
    out = []
    for name, shape in DT_SHAPES:
        for R_in in ((0.0, 0.03) if name in _PHI_SHAPES else (0.0,)):
            for f in DT_F:
                out.append(('%s-%dx%dx%d-%s-f%g' % ((name,) + shape + ('axis' if R_in == 0.0 else 'annulus', f)), (shape, R_in, f)))
    return out


def dt_case(shape, R_in, f):
    """Robin closures on r and on both z ends: a Robin end everywhere keeps the systems well conditioned at large f"""
    return make_case(shape, pair=('robin', 'robin'), R_in=R_in, mode='plain', dt=f * DR * DR / ALPHA)


@functools.lru_cache(maxsize=None)
def dt_reference(shape, R_in, f):
    """cyl_ref_ld after two steps, computed once per session: (longdouble field, the same rounded to float64); read-only"""
    ld = run_ref_ld(dt_case(shape, R_in, f))
    f64 = ld.astype(np.float64)
    ld.setflags(write=False); f64.setflags(write=False)
    return ld, f64
