"""Stage times of the STL correction of voxel Robin coefficients at scale: a formula mesh of 10^6 triangles (the side of a
tilted cylinder, 3.6 x 10^6 sub-triangles) inside a 512^3 all-true mask, dx = 1 mm -- the case of
tests/test_stlcorr_gpu.py::test_a_million_triangles_in_512_cubed.

    python scripts/stlcorr_probe.py [--rounds 15] [--out profiles/stlcorr_probe.json]

Stages, each between two events on the stream, warmed up twice, medians over the rounds: count (adi_stlcorr_count), scan
(torch.cumsum and the read of the slot total by the host), bin (adi_stlcorr_bin), sort (torch.sort, stable, 64-bit keys),
zero (the two output fields of one face), accumulate (adi_stlcorr_accumulate into that face), fallback
(adi_stlcorr_fallback, one face: a pass over the mask), and `whole`: build_corrected_fields for six faces as a user calls it,
mesh upload and the twelve zero-filled 1 GiB fields included, by the host clock around a synchronise.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from adi_thermal_fields_amd import _lib                                          # noqa: E402
from adi_thermal_fields_amd._lib import check, lib, ptr_array                    # noqa: E402
from adi_thermal_fields_amd.adi3d_hip_coeff import Layout                        # noqa: E402
from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh  # noqa: E402
from stlcorr_meshes import tube_triangles                                        # noqa: E402

STAGES = ('count', 'scan', 'bin', 'sort', 'zero', 'accumulate', 'fallback')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'stlcorr_probe needs a GPU'
    n, dx, ms_, eps = a.n, 1e-3, 6, 1e-16
    s = n / 512.0
    mesh = TriangleMesh(tube_triangles((0.256 * s, 0.256 * s, 0.256 * s), (0.3, 0.2, 1.0), 0.2 * s, 0.18 * s,
                                       int(1000 * s), int(500 * s), phase=0.01))
    dev = torch.device('cuda', torch.cuda.current_device())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = Layout(n, n, n)
    d_mask = L.to_layout(torch.ones((n, n, n), dtype=torch.uint8, device=dev), torch.uint8)
    tri = torch.from_numpy(mesh.triangles).to(dev)
    area = torch.from_numpy(mesh.area_faces).to(dev)
    nrm = torch.from_numpy(np.ascontiguousarray(mesh.face_normals)).to(dev)
    ntri = len(mesh)
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    face, base = 1, 250.0                                                        # 'x+'
    times = {k: [] for k in STAGES}
    nslot = 0
    for r in range(a.rounds + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        offset = torch.zeros(ntri + 1, dtype=torch.int64, device=dev)
        check(lib.adi_stlcorr_count(p(tri), p(area), ntri, dx, ms_, eps, ctypes.c_void_p(offset.data_ptr() + 8), stream()))
        ev[1].record()
        offset.cumsum_(0)
        nslot = int(offset[-1].item())
        ev[2].record()
        key = torch.empty(nslot, dtype=torch.int64, device=dev)
        sub = torch.empty(nslot, dtype=torch.float64, device=dev)
        st = torch.empty(nslot, dtype=torch.int64, device=dev)
        check(lib.adi_stlcorr_bin(p(tri), p(area), p(offset), ntri, nslot, p(d_mask), n, n, n, L.sx, L.pz, org, dx, ms_,
                                  p(key), p(sub), p(st), stream()))
        ev[3].record()
        ks, order = torch.sort(key, stable=True)
        ev[4].record()
        robin, scale = L.empty(zero=True), L.empty(zero=True)
        ev[5].record()
        tab = lambda t: ptr_array([t.data_ptr() if f == face else None for f in range(6)])
        check(lib.adi_stlcorr_accumulate(p(ks), p(order), p(sub), p(st), p(nrm), nslot, dx,
                                         (ctypes.c_double * 6)(*[base if f == face else 0.0 for f in range(6)]),
                                         ptr_array([None] * 6), tab(robin), tab(scale), stream()))
        ev[6].record()
        check(lib.adi_stlcorr_fallback(p(d_mask), n, n, n, L.sx, L.pz, face, base, p(robin), p(scale), stream()))
        ev[7].record()
        torch.cuda.synchronize()
        if r >= 2:
            for i, k in enumerate(STAGES):
                times[k].append(ev[i].elapsed_time(ev[i + 1]))
        del robin, scale, key, sub, st, ks, order
    corr = STLBoundaryCorrector(mesh, d_mask, (0.0, 0.0, 0.0), dx)
    h6 = {f: 250.0 for f in _lib.FACES}
    whole = []
    for r in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = corr.build_corrected_fields(h6)
        torch.cuda.synchronize()
        whole.append(1e3 * (time.perf_counter() - t0))
        del out
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = dict(shape=[n, n, n], triangles=ntri, sub_triangles=nslot, rounds=a.rounds, device=torch.cuda.get_device_name(),
               build_stamp=lib.adi_build_stamp().decode(), ms_median=med, ms_min={k: float(np.min(v)) for k, v in times.items()},
               ms_max={k: float(np.max(v)) for k, v in times.items()},
               ns_per_sub_triangle_count_to_accumulate=1e6 * sum(med[k] for k in ('count', 'scan', 'bin', 'sort', 'accumulate'))
               / max(nslot, 1),
               whole_six_faces_ms=[float(v) for v in whole[1:]], whole_six_faces_ms_median=float(np.median(whole[1:])),
               note='stages: device events, one face; whole: host clock around a synchronise, six faces, mesh upload and '
                    'zero-filled outputs included, first call dropped')
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
