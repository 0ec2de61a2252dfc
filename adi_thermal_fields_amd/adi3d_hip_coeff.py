"""adi3d_hip_coeff -- MI355X drop-in for the reference's Cartesian ADI backends.

Same operator surface as `adi3d_numba_coeff` / `adi3d_gpu_coeff` (the reference picks a backend by
module import, waam_from_stl_v7_mm.py:321-335), so a driver switches with

    import adi_thermal_fields_amd.adi3d_hip_coeff as adi

Names and meaning follow adi3d_numba_coeff.py:14-36, :38-55, :57-118, :290-302:
    Grid3D, Material, Params, AxisCoeffPack, exposed_mask, precompute_coeff_packs_unified,
    adi_step_hip_coeff  (also exported as adi_step_numba_coeff and adi_step_gpu_coeff).

Host code is Python; every number is computed by hand-written HIP kernels reached through the
ctypes C ABI of include/adi_hip.h.  PyTorch is used only for device memory and streams.
There is no CPU fallback.

Residency: a NumPy `Tn` is uploaded, stepped and downloaded (exact reference semantics: new array
out, input untouched).  Pass a `DeviceField` (see `to_device`) to keep the state in HBM across
steps -- the step then returns a new DeviceField, like the CuPy backend returns CuPy arrays.

Device layout: fields live in HBM with a padded plane stride (`Layout.sx`, chosen by
adi_recommended_plane_stride) so that the rows of an axis-0 line do not alias on the HBM channel
interleave; the C-order (nx, ny, nz) shape of the reference is what every host-visible view has.

Mask semantics: drivers rebind `grid.mask` and then rebuild the packs
(single_track_on_plate.py:159-163, waam_from_stl_v7_mm.py:494-495, :534).  The device copy of the
mask (and its neighbour-flags digest) is refreshed on every `grid.mask = ...` assignment AND on every
precompute_coeff_packs_unified(grid, ...) call, which is the documented synchronisation point.

Where things live: this module defines nothing, it re-exports.  fields.py -- Layout, DeviceField, to_device, Grid3D and the
device helpers; packs.py -- Material, Params, AxisCoeffPack, exposed_mask, precompute_coeff_packs_unified, MaterialMap (several
materials in one grid); heat_source.py --
GoldakSource, ScanPath, ScanPathSource and the one host definition of Goldak's double ellipsoid; deposition.py -- the surface impulse, the
perimeter ratio, birth_planes, BirthPacks, BeadProfile, PathDeposit (births along a scan path); surface_loss.py -- SurfaceLoss, LossPacks; phase.py -- PhaseChange, PhaseField, MaterialLaw, NonlinearPacks;
matmap_extras.py -- MapPhaseField, MapLossPacks (latent heat and surface loss with one law per material of a MaterialMap) and
MapSource (a moving GoldakSource inside the step of a MaterialMap), MapPathSource (a ScanPath inside it), MaterialTransitions (cells that change their material when
they get hot enough);
history.py -- HistoryLevels, ThermalHistory, SolidificationRecord; monitor.py -- FieldMonitor (probes, region extrema and sums; it
imports fields, packs and history, and step.py knows it by history._StepRecorder, the base the three recorders share); step.py --
the stage entry points, StepExtras (the record of the step's optional parts), the launch sequence, adi_step_hip_coeff,
StagedStepper.  Each imports only those before it in this list ("Module map"); code inside the package imports
from them, drivers and tests from here.
"""
import sys

from ._facade import ReExporting
from ._lib import lib, check, ptr_array
from .fields import (_MASK_VERSIONS, _device, _stream, _p, _sweep_workspace_bytes, recommended_dims, Layout, DeviceField,
                     to_device, Grid3D, _wrap)
from .packs import Material, Params, AxisCoeffPack, exposed_mask, _fc_arg, precompute_coeff_packs_unified, MaterialMap
from .heat_source import GoldakSource, ScanPath, ScanPathSource, _source_block, _source_work
from .deposition import (apply_surface_impulse_Q, exposed_faces_per_layer, count_exposed_faces, perimeter_ratio, birth_planes,
                         BirthPacks, BeadProfile, PathDeposit)
from .surface_loss import SurfaceLoss, LossPacks
from .phase import PhaseChange, PhaseField, MaterialLaw, NonlinearPacks
from .matmap_extras import MapPhaseField, MapLossPacks, MapSource, MapPathSource, MaterialTransitions
from .history import HistoryLevels, ThermalHistory, SolidificationRecord
from .monitor import FieldMonitor
from .step import (adi_explicit_rhs, adi_sweep_axis, adi_explicit_sweep_axis0, adi_step_hip_coeff, adi_step_numba_coeff,
                   adi_step_gpu_coeff, StagedStepper, fused_supported, valid_range, _sparse_arg, _sweep_into,
                   _explicit_sweep0_into, _explicit_src_into, _source_lines0_into)

__all__ = ['Grid3D', 'Material', 'Params', 'AxisCoeffPack', 'exposed_mask', 'precompute_coeff_packs_unified',
           'adi_step_hip_coeff', 'adi_step_numba_coeff', 'adi_step_gpu_coeff', 'DeviceField', 'to_device',
           'adi_explicit_rhs', 'adi_sweep_axis', 'StagedStepper', 'Layout', 'apply_surface_impulse_Q',
           'exposed_faces_per_layer', 'count_exposed_faces', 'perimeter_ratio', 'birth_planes', 'BirthPacks',
           'GoldakSource', 'ScanPath', 'SurfaceLoss', 'LossPacks', 'PhaseChange', 'PhaseField', 'HistoryLevels',
           'ThermalHistory']
# (ScanPathSource, BeadProfile, PathDeposit, MaterialLaw, NonlinearPacks, SolidificationRecord, MaterialMap, MapPhaseField, MapLossPacks, MapSource, MapPathSource, MaterialTransitions and FieldMonitor are exported like the names above but are not part of the pinned `__all__`)

# an assignment to a name above reaches the module that defined it (_facade.ReExporting)
sys.modules[__name__].__class__ = ReExporting
