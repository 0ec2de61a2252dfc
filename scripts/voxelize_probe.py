"""Time the solid voxeliser stage by stage on the GPU and write profiles/voxelize_probe.json.

    python scripts/voxelize_probe.py [--n 512] [--level 8] [--reps 9] [--out profiles/voxelize_probe.json]

Cases: (a) a geodesic sphere of 20 * 4^level triangles (level 8: 1.3 million) into n^3, rays along z; (b) the 12-triangle
box into n^3, the load-balance case: two triangles over n x n columns; (c) axis='majority' of both.  Per stage (count,
scan of the counts, toggle, prefix + expand) and for the whole call: medians of device-event times after two warm-up
rounds.  In the same run a hipMemsetAsync of the n^3-byte mask is timed: the expand pass writes the mask once, so a plain
fill of it is its floor.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from adi_thermal_fields_amd._lib import check, lib  # noqa: E402
from adi_thermal_fields_amd import voxelize as vox  # noqa: E402
import voxelize_ref as vr  # noqa: E402
from stlcorr_meshes import box_triangles  # noqa: E402


def _timed(fn, reps, warm=2):
    """median / min of device-event milliseconds over `reps` calls after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'reps': reps}


def _popcount(words):
    x = words.to(torch.int64) & 0xffffffff
    return int(sum(int(((x >> b) & 1).sum()) for b in range(32)))


def stages(tri_host, origin, dx, shape, axis, reps):
    dev = torch.device('cuda', torch.cuda.current_device())
    tri = torch.from_numpy(np.ascontiguousarray(tri_host)).to(dev)
    ntri = tri.shape[0]
    nx, ny, nz = shape
    org = (ctypes.c_double * 3)(*[float(v) for v in origin])
    p, st = vox._p, vox._stream
    nwords = ctypes.c_long(0)
    check(lib.adi_voxelize_words(nx, ny, nz, axis, ctypes.byref(nwords)))
    words = torch.zeros(nwords.value, dtype=torch.int32, device=dev)
    count = torch.zeros(ntri + 1, dtype=torch.int64, device=dev)
    offset = torch.zeros(ntri + 1, dtype=torch.int64, device=dev)
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    leaks = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}
    out['count'] = _timed(lambda: check(lib.adi_voxelize_count(p(tri), ntri, org, dx, nx, ny, nz, axis,
                                                               ctypes.c_void_p(count.data_ptr() + 8), st())), reps)
    out['scan'] = _timed(lambda: torch.cumsum(count, 0, out=offset), reps)
    nitem = int(offset[-1].item())
    toggle = lambda: check(lib.adi_voxelize_toggle(p(tri), p(offset), ntri, nitem, org, dx, nx, ny, nz, axis, p(words), st()))
    out['zero_words'] = _timed(lambda: words.zero_(), reps)
    out['toggle'] = _timed(toggle, reps)
    words.zero_()
    toggle()
    toggled = _popcount(words)
    saved = words.clone()

    def prefix_expand():
        check(lib.adi_voxelize_scan(p(words), nx, ny, nz, axis, p(mask), p(leaks), st()))
    # the prefix pass works in place; what it reads the second time is no toggle grid, but the bytes moved are the same
    out['prefix_expand'] = _timed(prefix_expand, reps)
    words.copy_(saved)
    leaks.zero_()
    prefix_expand()
    out.update(triangles=ntri, tiles=nitem, toggled_bits=toggled, solid=int(mask.sum()), leaks=int(leaks.item()),
               toggle_ns_per_toggled_bit=1e6 * out['toggle']['median_ms'] / max(1, toggled))
    return out


def whole(tri_host, origin, dx, shape, axis, reps):
    mesh = type('Mesh', (), {'triangles': tri_host})()
    tri = torch.from_numpy(np.ascontiguousarray(tri_host)).cuda()
    leaks = torch.zeros(3, dtype=torch.int32, device=tri.device)
    axes = (0, 1, 2) if axis == 'majority' else (axis,)

    def device_part():                      # what voxelize_solid does once the triangles are on the device
        masks = [vox._one_axis(tri, [float(v) for v in origin], dx, shape, a, leaks, s) for s, a in enumerate(axes)]
        if axis == 'majority':
            check(lib.adi_voxelize_majority(vox._p(masks[0]), vox._p(masks[1]), vox._p(masks[2]), masks[0].numel(),
                                            vox._p(masks[0]), vox._stream()))
    out = {'device': _timed(device_part, reps)}
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vox.voxelize_solid(mesh, origin, dx, shape, axis=axis, as_tensor=True)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    out['voxelize_solid_wall_ms'] = {'median_ms': statistics.median(wall), 'min_ms': min(wall), 'reps': 3,
                                     'note': 'host clock, includes the upload of the triangles'}
    return out


def memset_floor(nbytes, reps):
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    buf = torch.empty(nbytes, dtype=torch.uint8, device='cuda')

    def fill():
        rc = hip.hipMemsetAsync(ctypes.c_void_p(buf.data_ptr()), 0, nbytes, vox._stream())
        assert rc == 0, rc
    out = _timed(fill, reps)
    out['bytes'] = nbytes
    out['GBps'] = nbytes / out['median_ms'] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--level', type=int, default=8)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxelize_probe.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe needs a GPU'
    n, dx = a.n, 1e-3
    shape = (n, n, n)
    org = np.array([0.0123, -0.004, 0.0007])
    sphere, _, _ = vr.geodesic_polyhedron(org + 0.5 * n * dx + np.array([0.21, -0.13, 0.07]) * dx, 0.47 * n * dx, a.level)
    box = box_triangles(*[org[m] + np.array([3.3, n - 3.2]) * dx for m in range(3)])
    res = {'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'dx': dx,
           'memset_mask': memset_floor(n * n * n, a.reps), 'cases': {}}
    for name, tri in (('a_sphere_%d_triangles' % len(sphere), sphere), ('b_box_12_triangles', box)):
        c = {'axis2': stages(tri, org, dx, shape, 2, a.reps)}
        c['axis0'] = stages(tri, org, dx, shape, 0, a.reps)
        c['whole_axis2'] = whole(tri, org, dx, shape, 2, a.reps)
        c['c_whole_majority'] = whole(tri, org, dx, shape, 'majority', a.reps)
        for ax in ('axis2', 'axis0'):
            c[ax]['prefix_expand_over_memset'] = c[ax]['prefix_expand']['median_ms'] / res['memset_mask']['median_ms']
        res['cases'][name] = c
        print(name, json.dumps(c), flush=True)
    ca, cb = res['cases'].values()
    res['toggle_per_crossing_box_over_sphere'] = (cb['axis2']['toggle_ns_per_toggled_bit'] /
                                                  ca['axis2']['toggle_ns_per_toggled_bit'])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({'memset_mask': res['memset_mask'], 'ratio_b_over_a': res['toggle_per_crossing_box_over_sphere']}))


if __name__ == '__main__':
    main()
