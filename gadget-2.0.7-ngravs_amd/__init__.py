"""gadget-2.0.7-ngravs_amd -- host-side mirror of the reference's gravity entry points over the
C ABI of libngravs_hip.so (include/ngravs_hip.h).

The directory name is not an importable identifier; load it with `__graft_entry__.load_package()`
(importlib, alias `ngravs_amd`).  The names below follow the reference (proto.h): an `Engine`
plays the role of the globals P[]/All/TypeToGrav[] for one MPI task and exposes
domain_Decomposition(), force_treebuild(), gravity_tree(), pmforce_periodic(),
compute_accelerations().  There is NO CPU fallback: if the HIP library or a GPU is missing every
entry point raises (the oracle under oracle/ is test infrastructure and is never imported here).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi, ic  # noqa: F401
from .abi import (Config, Particles, Stats, make_config, WALK_GROUP, WALK_STRICT,  # noqa: F401
                  LAW_NONE, LAW_NEWTON, LAW_NEG_NEWTON, LAW_YUKAWA, LAW_COLOYUK, LAW_BAMBAM, LAW_SOURCEBAM, LAW_TARGETBAM)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libngravs_hip.so")
_LIB = None

# every symbol include/ngravs_hip.h declares (tests/test_abi.py checks the .so exports all of them)
EXPORTS = [
    "ngravs_abi_version", "ngravs_build_info", "ngravs_config_default", "ngravs_create", "ngravs_create_with_laws", "ngravs_destroy",
    "ngravs_last_walk_kernel", "ngravs_last_pm_cus", "ngravs_cu_probe", "ngravs_shortrange_table_with_laws", "ngravs_user_table_eval",
    "ngravs_create_with_lattice", "ngravs_user_lattice_table", "ngravs_create_with_potentials",
    "ngravs_set_fatal_handler", "ngravs_set_opening", "ngravs_set_walk_mode", "ngravs_set_softening", "ngravs_dd_record_bytes", "ngravs_get_config", "ngravs_set_tuning",
    "ngravs_memcpy", "ngravs_device_alloc", "ngravs_device_free",
    "ngravs_set_particles",
    "ngravs_set_old_acc", "ngravs_set_gas_softening", "ngravs_update_particles", "ngravs_force_update_tree", "ngravs_domain_decomposition", "ngravs_discard_grav_pm",
    "ngravs_force_treebuild", "ngravs_gravity_tree",
    "ngravs_pmforce_periodic", "ngravs_compute_accelerations", "ngravs_get_accel", "ngravs_get_stats", "ngravs_walk_unopened", "ngravs_walk_moment_skips",
    "ngravs_get_domain", "ngravs_get_keys", "ngravs_get_order", "ngravs_get_shard", "ngravs_last_error",
    "ngravs_peano_hilbert_key", "ngravs_peano_keys", "ngravs_shortrange_table", "ngravs_direct_sum", "ngravs_direct_sum_targets",
    "ngravs_dd_num_local", "ngravs_dd_local_extent", "ngravs_dd_set_extent", "ngravs_get_domain_extent", "ngravs_dd_set_toptree",
    "ngravs_dd_get_toptree", "ngravs_dd_peano_order", "ngravs_dd_leaf_sums", "ngravs_dd_target_bounds", "ngravs_dd_keep_margin", "ngravs_dd_pack", "ngravs_dd_get_dest",
    "ngravs_dd_pack_leaves", "ngravs_dd_set_top", "ngravs_dd_recv_buffer", "ngravs_dd_apply_migration", "ngravs_dd_set_halo",
    "ngravs_dd_leaf_sums_kept", "ngravs_dd_pack_leaves_kept", "ngravs_dd_refresh_halo", "ngravs_dd_update_top", "ngravs_dd_get_kept",
    "ngravs_dd_set_ids", "ngravs_dd_get_ids",
    "ngravs_pm_slab_begin", "ngravs_pm_slab_pack", "ngravs_pm_slab_unpack", "ngravs_pm_slab_bytes",
    "ngravs_sph_density", "ngravs_sph_kernel", "ngravs_sph_hydro", "ngravs_sph_accelerations",
    "ngravs_sph_hsml_guess", "ngravs_sph_density_sums", "ngravs_sph_hydro_sums", "ngravs_sph_density_update",
    "ngravs_gravity_tree_targets", "ngravs_pm_targets",
    "ngravs_time_tables", "ngravs_time_factors", "ngravs_next_sync_point", "ngravs_move_particles", "ngravs_displacement_sums",
    "ngravs_dt_displacement", "ngravs_advance_and_find_timesteps",
    "ngravs_global_sums", "ngravs_global_finish", "ngravs_energy_line",
    "ngravs_snapshot_plan", "ngravs_snapshot_block_count", "ngravs_snapshot_block", "ngravs_snapshot_header", "ngravs_snapshot_write",
    "ngravs_find_next_outputtime",
    "ngravs_compute_potential", "ngravs_potential_targets", "ngravs_lattice_potential_table", "ngravs_last_potential_ms",
]
# include/ngravs_host.h (plain-C multi-task drivers over a communicator vtable, linked into the same library)
HOST_EXPORTS = ["ngravs_host_comm_selftest", "ngravs_host_kept_step", "ngravs_host_toptree_borrow", "ngravs_host_domain_decomposition", "ngravs_host_domain_owners", "ngravs_host_domain_halo",
                "ngravs_host_plan_free", "ngravs_host_pmforce_periodic", "ngravs_host_compute_accelerations", "ngravs_host_split",
                "ngravs_host_pm_seconds", "ngravs_host_toptree_init", "ngravs_host_toptree_from_children", "ngravs_host_toptree_adapt",
                "ngravs_host_toptree_free", "ngravs_host_import_request", "ngravs_host_import_request_margin"]
# include/ngravs_comm_rccl.h (libngravs_rccl.so: the communicator vtable over RCCL, plain C)
RCCL_LIB_PATH = os.path.join(_HERE, "libngravs_rccl.so")
RCCL_EXPORTS = ["ngravs_rccl_selftest", "ngravs_rccl_unique_id", "ngravs_rccl_create", "ngravs_rccl_fill", "ngravs_rccl_destroy", "ngravs_rccl_stats",
                "ngravs_rccl_last_error", "ngravs_rccl_world", "ngravs_rccl_barrier", "ngravs_rccl_set_timeout"]


class NgravsError(RuntimeError):
    pass


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libngravs_hip.so (in-tree)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise NgravsError("libngravs_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.ngravs_build_info.restype = C.c_char_p
        L.ngravs_last_error.restype = C.c_char_p
        L.ngravs_last_error.argtypes = [C.c_void_p]
        L.ngravs_peano_hilbert_key.restype = C.c_int64
        L.ngravs_peano_hilbert_key.argtypes = [C.c_int] * 4
        L.ngravs_force_treebuild.restype = C.c_int64
        L.ngravs_force_treebuild.argtypes = [C.c_void_p]
        for name in ("ngravs_destroy", "ngravs_domain_decomposition", "ngravs_gravity_tree",
                     "ngravs_pmforce_periodic", "ngravs_discard_grav_pm"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.ngravs_compute_accelerations.argtypes = [C.c_void_p, C.c_int]
        L.ngravs_set_opening.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.ngravs_set_walk_mode.argtypes = [C.c_void_p, C.c_int]
        L.ngravs_set_softening.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_dd_record_bytes.restype = C.c_int64
        L.ngravs_dd_record_bytes.argtypes = [C.c_void_p, C.c_int]
        L.ngravs_set_particles.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_set_old_acc.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.ngravs_set_gas_softening.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.ngravs_get_accel.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_int, C.c_int]
        L.ngravs_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.ngravs_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.ngravs_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_get_domain.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_get_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ngravs_get_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ngravs_get_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_peano_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        L.ngravs_shortrange_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_direct_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.ngravs_direct_sum_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.ngravs_dd_local_extent.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_dd_set_extent.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_get_config.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_host_split.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p]
        L.ngravs_dd_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_host_toptree_init.argtypes = [C.c_void_p, C.c_int]
        L.ngravs_host_toptree_from_children.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.ngravs_host_toptree_adapt.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        L.ngravs_host_toptree_free.argtypes = [C.c_void_p]
        L.ngravs_host_toptree_free.restype = None
        L.ngravs_host_import_request.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ngravs_dd_apply_migration.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.ngravs_dd_set_halo.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.ngravs_dd_set_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ngravs_create_with_laws.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ngravs_last_walk_kernel.argtypes = [C.c_void_p]
        L.ngravs_last_pm_cus.argtypes = [C.c_void_p]
        L.ngravs_cu_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ngravs_shortrange_table_with_laws.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ngravs_user_table_eval.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p]
        L.ngravs_dd_get_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ngravs_create_with_lattice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.ngravs_user_lattice_table.argtypes = [abi.LATTICE_FN, C.c_double, C.c_void_p]
        L.ngravs_create_with_potentials.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.ngravs_sph_density.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_sph_kernel.argtypes = [C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.ngravs_sph_hydro.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_sph_accelerations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_sph_hsml_guess.argtypes = abi.SPH_HSML_GUESS_ARGTYPES
        L.ngravs_sph_density_sums.argtypes = abi.SPH_DENSITY_SUMS_ARGTYPES
        L.ngravs_sph_hydro_sums.argtypes = abi.SPH_HYDRO_SUMS_ARGTYPES
        L.ngravs_sph_density_update.argtypes = abi.SPH_DENSITY_UPDATE_ARGTYPES
        L.ngravs_sph_density_update.restype = C.c_int64
        L.ngravs_gravity_tree_targets.argtypes = abi.GRAVITY_TREE_TARGETS_ARGTYPES
        L.ngravs_pm_targets.argtypes = abi.PM_TARGETS_ARGTYPES
        L.ngravs_time_tables.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_time_factors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.ngravs_next_sync_point.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.ngravs_move_particles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.ngravs_displacement_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_dt_displacement.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.ngravs_advance_and_find_timesteps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        L.ngravs_global_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.ngravs_global_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.ngravs_energy_line.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64]
        L.ngravs_snapshot_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ngravs_snapshot_block_count.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.ngravs_snapshot_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32]
        L.ngravs_snapshot_header.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
        L.ngravs_snapshot_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int64, C.c_char_p]
        L.ngravs_find_next_outputtime.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.ngravs_compute_potential.argtypes = abi.COMPUTE_POTENTIAL_ARGTYPES
        L.ngravs_potential_targets.argtypes = abi.POTENTIAL_TARGETS_ARGTYPES
        L.ngravs_lattice_potential_table.argtypes = abi.LATTICE_POTENTIAL_TABLE_ARGTYPES
        L.ngravs_last_potential_ms.argtypes = [C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def shard_range(n, rank, world_size):
    """Target shard of `rank`: positions [first, first+count) of the Peano order, cut on wave (64) boundaries so
    that target groups are identical for every world size (mirrors ngravs_domain_decomposition in capi.hip; the
    role of DomainMyStart/DomainMyLast after domain_findSplit, reference domain.c:347-456)."""
    lo = (n * rank) // world_size
    hi = (n * (rank + 1)) // world_size
    lo = (lo // 64) * 64
    hi = n if rank + 1 == world_size else (hi // 64) * 64
    return lo, hi - lo


def peano_hilbert_key(x, y, z, bits):
    """peano_hilbert_key() (reference peano.c:356-398), host implementation of the library."""
    return int(lib().ngravs_peano_hilbert_key(int(x), int(y), int(z), int(bits)))


def shortrange_table(cfg):
    """shortrange_fourier_force/pot[target][source][NTAB] (reference forcetree.c:3246-3403)."""
    ng = cfg.n_gravs
    force = np.zeros((ng, ng, abi.NTAB))
    pot = np.zeros((ng, ng, abi.NTAB))
    rc = lib().ngravs_shortrange_table(C.byref(cfg), force.ctypes.data, pot.ctypes.data)
    if rc != 0:
        raise NgravsError("ngravs_shortrange_table: %d" % rc)
    return force, pot


def shortrange_table_with_laws(cfg, user_fns):
    """shortrange_table() where law_normed may hold user ids: user_fns = [(abi.USER_NORMED, f), ...]; no GPU needed"""
    arr, nfns, keep = abi.user_registry(user_fns)
    ng = cfg.n_gravs
    force = np.zeros((ng, ng, abi.NTAB))
    pot = np.zeros((ng, ng, abi.NTAB))
    rc = lib().ngravs_shortrange_table_with_laws(C.byref(cfg), arr, nfns, force.ctypes.data, pot.ctypes.data)
    del keep
    if rc != 0:
        raise NgravsError("ngravs_shortrange_table_with_laws: %d" % rc)
    return force, pot


def user_table_eval(kind, fn, r, r_lo=0.0, r_hi=0.0, h=0.0):
    """what the kernels evaluate for a user law, built and evaluated on the host (no GPU): kind USER_ACCEL -> accel(1,1,r^2,r,1)
    from the table over [r_lo, r_hi]; USER_SPLINE -> spline(1,1,h,r,1) from the table of softening h; USER_POT -> pot(1,1,0,r,1)
    and USER_POT_SPLINE -> pot_spline(1,1,h,r,1) of a user_potentials entry in the same way.  Returns (values, the largest
    relative deviation the fit saw at its check points)."""
    arr, _, keep = abi.user_registry([(kind, fn)])
    r = np.ascontiguousarray(r, dtype=np.float64)
    out = np.zeros_like(r)
    err = C.c_double(0)
    rc = lib().ngravs_user_table_eval(arr, r_lo, r_hi, h, r.ctypes.data, len(r), out.ctypes.data, C.byref(err))
    del keep
    if rc != 0:
        raise NgravsError("ngravs_user_table_eval: %d" % rc)
    return out, err.value


def user_lattice_table(fn, box_size):
    """one lattice-correction table as the kernels read it, built on the host (no GPU): fn (abi.LATTICE_FN or a Python callable
    fn(i, j, k, x, force)) sampled at x = 0.5 (i, j, k) / 64 and divided by box_size^2; shape (3, 65, 65, 65)"""
    w = abi.lattice_fn(fn)
    out = np.zeros((3, abi.LAT_EN1, abi.LAT_EN1, abi.LAT_EN1))
    rc = lib().ngravs_user_lattice_table(w, float(box_size), out.ctypes.data)
    if rc != 0:
        msg = lib().ngravs_last_error(None)
        raise NgravsError("ngravs_user_lattice_table: %d: %s" % (rc, msg.decode() if msg else ""))
    return out


def sph_kernel(h, r):
    """(wk, dwk): the SPH spline and its derivative at radii r for smoothing length h, as the device code evaluates them
    (density.c:541-550; 0 where r >= h); no GPU needed"""
    r = np.ascontiguousarray(r, dtype=np.float64)
    wk, dwk = np.zeros_like(r), np.zeros_like(r)
    rc = lib().ngravs_sph_kernel(float(h), r.ctypes.data, r.size, wk.ctypes.data, dwk.ctypes.data)
    if rc != 0:
        raise NgravsError("ngravs_sph_kernel: %d" % rc)
    return wk, dwk


def hydro_factors(time, omega0, omega_lambda, hubble, gamma=5.0 / 3):
    """(hubble_a2, fac_mu, fac_vsic_fix) of a comoving run at expansion factor `time` (hydra.c:78-97), for
    Engine.sph_hydro(..., comoving=...); no GPU needed"""
    hubble_a = omega0 / (time * time * time) + (1 - omega0 - omega_lambda) / (time * time) + omega_lambda
    hubble_a = hubble * np.sqrt(hubble_a)
    hubble_a2 = time * time * hubble_a
    fac_mu = np.power(time, 3 * (gamma - 1) / 2) / time
    fac_vsic_fix = hubble_a * np.power(time, 3 * (gamma - 1))
    return float(hubble_a2), float(fac_mu), float(fac_vsic_fix)


def time_tables(par, rule=0):
    """init_drift_table() of the reference (driftfac.c:26-60) for the cosmology and the time span of par
    (abi.make_time_params): (drift, gravkick, hydrokick), abi.DRIFT_TABLE_LENGTH float64 each.  rule 0: the library's rule,
    1: its finer check rule.  No GPU needed."""
    t = [np.zeros(abi.DRIFT_TABLE_LENGTH) for _ in range(3)]
    rc = lib().ngravs_time_tables(C.byref(par), int(rule), *(x.ctypes.data for x in t))
    if rc != 0:
        raise NgravsError("ngravs_time_tables: %d" % rc)
    return tuple(t)


def time_factors(par, ti0, ti1):
    """(get_drift_factor, get_gravkick_factor, get_hydrokick_factor)(ti0, ti1) (driftfac.c:67-174) from the tables in par; no
    GPU needed"""
    out = np.zeros(3)
    rc = lib().ngravs_time_factors(C.byref(par), int(ti0), int(ti1), out.ctypes.data)
    if rc != 0:
        raise NgravsError("ngravs_time_factors: %d" % rc)
    return tuple(float(x) for x in out)


def dt_displacement(par, sums, G, asmth, time):
    """find_dt_displacement_constraint() after its sums (timestep.c:595-659); asmth = All.Asmth[0], 0 without a mesh; time =
    All.Time.  No GPU needed."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    assert sums.shape == (18,)
    out = C.c_double(0)
    rc = lib().ngravs_dt_displacement(C.byref(par), sums.ctypes.data, float(G), float(asmth), float(time), C.byref(out))
    if rc != 0:
        raise NgravsError("ngravs_dt_displacement: %d" % rc)
    return float(out.value)


def global_finish(sums):
    """compute_global_quantities_of_system() after its MPI_Reduce (global.c:130-194) from the (all-reduced) 78 sums of
    Engine.global_sums: abi.SysState, the reference's struct state_of_system.  No GPU needed."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    assert sums.shape == (abi.GLOBAL_NSUMS,)
    out = abi.SysState()
    rc = lib().ngravs_global_finish(sums.ctypes.data, C.byref(out))
    if rc != 0:
        raise NgravsError("ngravs_global_finish: %d" % rc)
    return out


def energy_line(state, time):
    """the line energy_statistics() appends to energy.txt (run.c:419-429) for an abi.SysState at All.Time = time.  No GPU needed."""
    buf = C.create_string_buffer(1024)
    rc = lib().ngravs_energy_line(C.byref(state), float(time), buf, len(buf))
    if rc < 0:
        raise NgravsError("ngravs_energy_line: %d" % rc)
    return buf.raw[:rc].decode()


def find_next_outputtime(par, rule, ti_curr):
    """find_next_outputtime(ti_curr) of the reference (run.c:244-361) for an abi.OutputRule (abi.make_output_rule): the first
    output time >= ti_curr on the integer time line, 2 * abi.TIMEBASE when there is none.  Raises NgravsError where the reference
    ends with 13123, 110 or 111.  No GPU needed."""
    out = C.c_int32(0)
    rc = lib().ngravs_find_next_outputtime(C.byref(par), C.byref(rule), int(ti_curr), C.byref(out))
    if rc != 0:
        msg = lib().ngravs_last_error(None)
        raise NgravsError("ngravs_find_next_outputtime failed: status %d (%s)" % (rc, msg.decode() if msg else ""))
    return int(out.value)


def snapshot_header(par, npart, time, mass_table=None, npart_total=None, num_files=1, hubble_param=0.0, box_size=0.0):
    """struct io_header as write_file fills it (io.c:720-761): 256 bytes.  No GPU needed."""
    s = abi.Snapshot()
    s.mass_table = (C.c_double * 6)(*([0.0] * 6 if mass_table is None else [float(x) for x in mass_table]))
    s.box_size, s.hubble_param = float(box_size), float(hubble_param)
    npart = np.ascontiguousarray(npart, dtype=np.int64)
    total = npart if npart_total is None else np.ascontiguousarray(npart_total, dtype=np.int64)
    assert npart.shape == (6,) and total.shape == (6,)
    out = C.create_string_buffer(256)
    rc = lib().ngravs_snapshot_header(C.byref(par), C.byref(s), npart.ctypes.data, total.ctypes.data, int(num_files), float(time), out)
    if rc != 0:
        raise NgravsError("ngravs_snapshot_header: %d" % rc)
    return out.raw


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _is_device(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _columns(cols, shapes, on_device, int_keys=(), own=()):
    """the arrays of one call, all of one kind: numpy (converted to contiguous float64 / int32) or torch tensors on the device
    (float64 / int32, contiguous, as they are).  own: the keys of arrays that the library writes through, which must be right as
    they are: the caller's own arrays, never converted copies.  Returns the dict and the function that gives an array's address."""
    given = cols
    if on_device:
        import torch
        for k, a in cols.items():
            assert a is None or (a.dtype == (torch.int32 if k in int_keys else torch.float64) and a.is_contiguous() and a.is_cuda), k
        torch.cuda.synchronize()   # the library works on a stream of its own: the tensors must be complete
        addr = lambda a: a.data_ptr()   # noqa: E731
    else:
        cols = {k: a if a is None else np.ascontiguousarray(a, dtype=np.int32 if k in int_keys else np.float64) for k, a in cols.items()}
        addr = lambda a: a.ctypes.data   # noqa: E731
    for k in own:
        assert cols[k] is given[k], k + " must be a C-contiguous float64 (int32) numpy array: it is written through"
    for k, a in cols.items():
        assert a is None or tuple(a.shape) == shapes[k], (k, tuple(a.shape), shapes[k])
    return cols, addr


def _zeros(shape, like, on_device, dtype=np.float64):
    if on_device:
        import torch
        return torch.zeros(shape, dtype=torch.int32 if dtype == np.int32 else torch.float64, device=like.device)
    return np.zeros(shape, dtype=dtype)


def _results(names, shape, out, like, on_device):
    """the arrays a call writes: what `out` holds under a name (written through), else zeros"""
    return {k: out[k] if out and k in out else _zeros(shape(k), like, on_device) for k in names}


def _set_columns(st, cols, addr):
    """address and row stride of every given array into the fields <key> and <key>_stride of an ABI struct"""
    for k, a in cols.items():
        if a is not None:
            setattr(st, k, addr(a))
            setattr(st, k + "_stride", (4 if str(a.dtype).endswith("int32") else 8) * (3 if len(a.shape) == 2 else 1))


def _hydro_switches(st, art_bulk_visc_const, timebase_interval, gamma, viscosity_limiter, comoving, on_device):
    """the switch fields that abi.HydroIn and abi.GasIn share"""
    st.art_bulk_visc_const, st.timebase_interval, st.gamma = float(art_bulk_visc_const), float(timebase_interval), float(gamma)
    st.viscosity_limiter, st.on_device = int(bool(viscosity_limiter)), int(on_device)
    if comoving is not None:
        st.comoving = 1
        st.hubble_a2, st.fac_mu, st.fac_vsic_fix = (float(x) for x in comoving)


def sph_density_update(sums, hsml, left, right, rounds, des_num_ngb, max_num_ngb_deviation, min_gas_hsml=0.0):
    """The owner's side of one round of density() (density.c:296-389) for targets whose added sums [n,7] came from
    Engine.sph_density_sums: hsml, left, right (float64 [n]) and rounds (int32 [n]) are UPDATED IN PLACE (left = right = 0,
    rounds = 0 before the first round).  numpy arrays (no GPU needed) or torch tensors on the device.  Returns a dict: accepted
    (int32 [n]), hsml, density, num_ngb, div_vel, curl_vel, dhsml_factor (written for accepted targets, else 0), failed (the
    number of targets past MAXITER)."""
    on_device = _is_device(sums)
    n = int(sums.shape[0])
    io = dict(sums=sums, hsml=hsml, left=left, right=right, rounds=rounds)
    chk, addr = _columns(io, dict(sums=(n, 7), hsml=(n,), left=(n,), right=(n,), rounds=(n,)), on_device, int_keys=("rounds",),
                         own=("hsml", "left", "right", "rounds"))
    res = {"accepted": _zeros(n, sums, on_device, np.int32)}
    uo = abi.SphUpdateOut()
    uo.accepted = addr(res["accepted"])
    for k in abi.SPH_UPDATE_NAMES:
        res[k] = _zeros(n, sums, on_device)
        setattr(uo, k, addr(res[k]))
    rc = lib().ngravs_sph_density_update(n, addr(chk["sums"]), addr(hsml), addr(left), addr(right), addr(rounds), float(des_num_ngb),
                                         float(max_num_ngb_deviation), float(min_gas_hsml), C.byref(uo), int(on_device))
    if rc < 0:
        msg = lib().ngravs_last_error(None)
        raise NgravsError("ngravs_sph_density_update failed: status %d (%s)" % (rc, msg.decode() if msg else ""))
    res["failed"] = int(rc)
    return res


class Engine:
    """One task's gravity state: the replacement for the reference's globals on this path."""

    def __init__(self, cfg, user_fns=None, user_lattice=None, user_potentials=None):
        """user_fns: [(abi.USER_ACCEL | USER_SPLINE | USER_GREENS | USER_NORMED, f), ...], f(target, source, r2_or_h_or_k2,
        r_or_k, N) -> float; entry k is wired as abi.LAW_USER0 + k / abi.SPLINE_USER0 + k.  user_lattice: [(target, source,
        fn), ...], the lattice correction of a pair wired with a user accel id in a periodic run (the reference's
        LatticeForce[target][source]): fn is an abi.LATTICE_FN (e.g. from the model's shared library) or a Python callable
        fn(i, j, k, x, force), which is slow here -- 65^3 = 274 625 calls, serialised by the GIL.  user_potentials: [(target,
        source, pot, pot_spline, lattice_pot or None, lattice_zero), ...], the potential companions of a pair (the reference's
        PotentialFxns, PotentialSplines, LatticePotential, LatticeZero [target][source]) for compute_potential() and
        potential_targets(): pot and pot_spline as the laws of user_fns, lattice_pot an abi.LATTICE_POT_FN or a Python callable
        fn(x) -> float.  The callbacks are kept alive with the engine (the library calls them when it (re)builds its tables)."""
        self.cfg = cfg
        self._h = C.c_void_p()
        self._user_arr, nfns, self._user_keep = abi.user_registry(user_fns)
        self._lat_arr, nlat, self._lat_keep = abi.lattice_registry(user_lattice)
        self._pot_arr, npot, self._pot_keep = abi.potential_registry(user_potentials)
        rc = lib().ngravs_create_with_potentials(C.byref(cfg), self._user_arr, nfns, self._lat_arr, nlat, self._pot_arr, npot,
                                                 C.byref(self._h))
        if rc != 0:
            msg = lib().ngravs_last_error(None)
            self.status = rc
            raise NgravsError("ngravs_create failed with status %d (no HIP device or bad wiring): %s" % (rc, msg.decode() if msg else ""))
        self._keep = []
        self.n = 0

    def last_walk_kernel(self):
        """abi.KERNEL_*: the kernel the last gravity_tree() walked with"""
        return int(lib().ngravs_last_walk_kernel(self._h))

    def last_pm_cus(self):
        """CUs reserved for PM beside the walk in the last compute_accelerations() (0: one after another)"""
        return int(lib().ngravs_last_pm_cus(self._h))

    def cu_probe(self, which, nblocks=2048):
        """ids (XCC << 8 | CU/SH/SE bits of HW_ID) of the CUs nblocks workgroups ran on: which = 0 the context's stream,
        1 the PM stream, 2 the walk stream of the overlapped step"""
        out = np.zeros(nblocks, dtype=np.int32)
        self._check(lib().ngravs_cu_probe(self._h, which, nblocks, out.ctypes.data), "ngravs_cu_probe")
        return out

    def close(self):
        if self._h:
            lib().ngravs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().ngravs_last_error(self._h)
            raise NgravsError("%s failed: status %d (%s)" % (what, rc, msg.decode() if msg else ""))

    # -- P[] hand-over ------------------------------------------------------------------------
    def _host_columns(self, pos, mass, ptype, old_acc, active, grav_pm, grav_cost=None):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        ptype = np.ascontiguousarray(ptype, dtype=np.int32)
        p = Particles()
        p.n = len(pos)
        p.pos, p.pos_stride = pos.ctypes.data, 24
        p.mass, p.mass_stride = mass.ctypes.data, 8
        p.type, p.type_stride = ptype.ctypes.data, 4
        keep = [pos, mass, ptype]
        if old_acc is not None:
            old_acc = np.ascontiguousarray(old_acc, dtype=np.float64)
            p.old_acc, p.old_acc_stride = old_acc.ctypes.data, 8
            keep.append(old_acc)
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.uint8)
            p.active, p.active_stride = active.ctypes.data, 1
            keep.append(active)
        if grav_pm is not None:
            grav_pm = np.ascontiguousarray(grav_pm, dtype=np.float64)
            p.grav_pm, p.grav_pm_stride = grav_pm.ctypes.data, 24
            keep.append(grav_pm)
        if grav_cost is not None:
            grav_cost = np.ascontiguousarray(grav_cost, dtype=np.float32)
            p.grav_cost, p.grav_cost_stride = grav_cost.ctypes.data, 4
            keep.append(grav_cost)
        p.on_device = 0
        self._keep = keep
        return p

    def set_particles(self, pos, mass, ptype, old_acc=None, active=None, grav_pm=None, grav_cost=None):
        """numpy (host) columns (the fields of P[] the path reads); grav_pm = P[].GravPM of the last PM step, if any;
        grav_cost = P[].GravCost (the work weight of the multi-task domain cut)"""
        p = self._host_columns(pos, mass, ptype, old_acc, active, grav_pm, grav_cost)
        self.n = p.n
        self._check(lib().ngravs_set_particles(self._h, C.byref(p)), "ngravs_set_particles")

    def update_particles(self, pos, mass, ptype, old_acc=None, active=None):
        """same particles, new positions / OldAcc / active flags: the decomposition and the tree topology are kept
        (drifted tree, TreeDomainUpdateFrequency > 0); gravity_tree() / pmforce_periodic() refit the nodes first"""
        p = self._host_columns(pos, mass, ptype, old_acc, active, None)
        self._check(lib().ngravs_update_particles(self._h, C.byref(p)), "ngravs_update_particles")

    def force_update_tree(self):
        self._check(lib().ngravs_force_update_tree(self._h), "ngravs_force_update_tree")

    def set_particles_device(self, n, pos_ptr, mass_ptr, type_ptr, old_acc_ptr=None, active_ptr=None, grav_pm_ptr=None):
        """HIP device pointers (e.g. torch tensors' data_ptr()): zero-copy hand-over."""
        p = Particles()
        p.n = n
        p.pos, p.pos_stride = pos_ptr, 24
        p.mass, p.mass_stride = mass_ptr, 8
        p.type, p.type_stride = type_ptr, 4
        if old_acc_ptr:
            p.old_acc, p.old_acc_stride = old_acc_ptr, 8
        if active_ptr:
            p.active, p.active_stride = active_ptr, 1
        if grav_pm_ptr:
            p.grav_pm, p.grav_pm_stride = grav_pm_ptr, 24
        p.on_device = 1
        self.n = n
        self._check(lib().ngravs_set_particles(self._h, C.byref(p)), "ngravs_set_particles")

    def set_old_acc(self, old_acc):
        old_acc = np.ascontiguousarray(old_acc, dtype=np.float64)
        self._check(lib().ngravs_set_old_acc(self._h, old_acc.ctypes.data, 8, 0), "ngravs_set_old_acc")

    def set_old_acc_device(self, ptr):
        """OldAcc from a HIP device pointer (N contiguous doubles, caller order)"""
        self._check(lib().ngravs_set_old_acc(self._h, ptr, 8, 1), "ngravs_set_old_acc")

    def set_gas_softening(self, hsml):
        """adaptive gravitational softening for gas (ADAPTIVE_GRAVSOFT_FORGAS): one length per own row, caller order; rows that
        are not type 0 are never read.  hsml: a numpy array, a device tensor (float64, contiguous), or None to switch back to the
        lengths per type"""
        if hsml is None:
            rc = lib().ngravs_set_gas_softening(self._h, None, 0, 0)
        elif hasattr(hsml, "data_ptr"):
            if str(hsml.dtype) != "torch.float64" or not hsml.is_contiguous() or hsml.numel() != self.n:
                raise ValueError("set_gas_softening: a device tensor must hold n contiguous float64 values")
            rc = lib().ngravs_set_gas_softening(self._h, hsml.data_ptr(), 8, 1 if hsml.is_cuda else 0)
        else:
            hsml = np.ascontiguousarray(hsml, dtype=np.float64)
            if hsml.shape != (self.n,):
                raise ValueError("set_gas_softening: one value per particle")
            rc = lib().ngravs_set_gas_softening(self._h, hsml.ctypes.data, 8, 0)
        self._check(rc, "ngravs_set_gas_softening")

    def get_old_acc_device(self, ptr):
        """write OldAcc (caller order) to a HIP device pointer"""
        self._check(lib().ngravs_get_accel(self._h, None, 0, None, 0, ptr, 8, None, 0, 1, 0), "ngravs_get_accel")

    def get_accel_device(self, acc_ptr=None, pm_ptr=None, old_ptr=None, cost_ptr=None, only_active=False):
        self._check(lib().ngravs_get_accel(self._h, acc_ptr, 24, pm_ptr, 24, old_ptr, 8, cost_ptr, 4, 1, int(only_active)),
                    "ngravs_get_accel")

    def walk_unopened(self):
        """top leaves the last group walk wanted opened but used as monopoles because they were not imported (multi-task trees)"""
        v = C.c_int64(0)
        self._check(lib().ngravs_walk_unopened(self._h, C.byref(v)), "ngravs_walk_unopened")
        return int(v.value)

    def walk_moment_skips(self):
        """(skips, within_reach) of the last group walk's traversal: nodes opened from the node head alone, their moments never
        fetched, out of the nodes within reach of their group; (0, 0) when the walk ran without the head"""
        s, w = C.c_int64(0), C.c_int64(0)
        self._check(lib().ngravs_walk_moment_skips(self._h, C.byref(s), C.byref(w)), "ngravs_walk_moment_skips")
        return int(s.value), int(w.value)

    def set_opening(self, theta, err_tol_force_acc):
        self._check(lib().ngravs_set_opening(self._h, theta, err_tol_force_acc), "ngravs_set_opening")
        self.cfg.err_tol_theta = theta
        self.cfg.err_tol_force_acc = err_tol_force_acc

    def set_softening(self, force_softening):
        """All.ForceSoftening[6] after set_softenings() (gravtree.c:468-518): comoving runs change it every step"""
        fs = np.ascontiguousarray(force_softening, dtype=np.float64)
        assert fs.shape == (6,)
        self._check(lib().ngravs_set_softening(self._h, fs.ctypes.data), "ngravs_set_softening")
        for t in range(6):
            self.cfg.force_softening[t] = fs[t]

    def set_walk_mode(self, mode):
        self._check(lib().ngravs_set_walk_mode(self._h, mode), "ngravs_set_walk_mode")

    def set_tuning(self, **kw):
        """ngravs_set_tuning(): e.g. set_tuning(walk_lcap=1024, walk_compact=0)"""
        for k, v in kw.items():
            self._check(lib().ngravs_set_tuning(self._h, k.encode(), float(v)), "ngravs_set_tuning(%s)" % k)

    # -- the reference's entry points (proto.h names) ---------------------------------------------
    def domain_Decomposition(self):
        self._check(lib().ngravs_domain_decomposition(self._h), "domain_Decomposition")

    def force_treebuild(self):
        nn = lib().ngravs_force_treebuild(self._h)
        if nn < 0:
            self._check(int(nn), "force_treebuild")
        return int(nn)

    def gravity_tree(self):
        self._check(lib().ngravs_gravity_tree(self._h), "gravity_tree")

    def pmforce_periodic(self):
        self._check(lib().ngravs_pmforce_periodic(self._h), "pmforce_periodic")

    def compute_accelerations(self, pm_step=True):
        self._check(lib().ngravs_compute_accelerations(self._h, 1 if pm_step else 0), "compute_accelerations")

    # -- results -------------------------------------------------------------------------------------
    def get_accel(self, want_pm=False, into=None):
        """(GravAccel[N,3], OldAcc[N], GravCost[N]) [+ GravPM[N,3]] in the caller's particle order.
        into=(acc, old, cost): write ONLY the rows of active particles into these existing arrays, as the reference
        does with P[] (gravtree.c:318-341); otherwise fresh arrays, rows that were not walked read 0 / the input OldAcc."""
        n = self.n
        if into is not None:
            acc, old, cost = into
            assert acc.dtype == np.float64 and old.dtype == np.float64 and cost.dtype == np.float32
            assert acc.flags.c_contiguous and old.flags.c_contiguous and cost.flags.c_contiguous
        else:
            acc = np.zeros((n, 3))
            old = np.zeros(n)
            cost = np.zeros(n, dtype=np.float32)
        pm = np.zeros((n, 3)) if want_pm else None
        self._check(lib().ngravs_get_accel(self._h, acc.ctypes.data, 24, _ptr(pm), 24, old.ctypes.data, 8,
                                           cost.ctypes.data, 4, 0, 1 if into is not None else 0), "ngravs_get_accel")
        return (acc, old, cost, pm) if want_pm else (acc, old, cost)

    def get_pm(self):
        pm = np.zeros((self.n, 3))
        self._check(lib().ngravs_get_accel(self._h, None, 0, pm.ctypes.data, 24, None, 0, None, 0, 0, 0), "ngravs_get_accel")
        return pm

    def _rows(self, k):
        """shape of the SPH column k over the rows of the last hand-over"""
        return (self.n, 3) if k in ("vel_pred", "hydro_accel") else (self.n,)

    def sph_density(self, vel, hsml, des_num_ngb, max_num_ngb_deviation, min_gas_hsml=0.0, out=None):
        """density() of the reference for one task (density.c:56-441): vel = SphP[].VelPred[N,3], hsml = starting guesses [N], one
        row per particle of the last hand-over (only rows of active type-0 particles are read as targets and written).  numpy
        arrays, or torch tensors on the device (float64, contiguous: no copy through the host).  Returns a dict: hsml, density,
        num_ngb, div_vel, curl_vel, dhsml_factor (rows that are no targets: the given hsml, else 0 -- or what `out`, a dict of
        arrays of the same kind, held), max_rounds, kernel_ms."""
        on_device = _is_device(vel)
        res = {"hsml": hsml.clone() if on_device else np.array(hsml, dtype=np.float64)}
        res.update(_results(abi.SPH_OUT_NAMES, self._rows, out, vel, on_device))
        cols, addr = _columns(dict(res, vel_pred=vel), {k: self._rows(k) for k in ["vel_pred"] + list(res)}, on_device, own=tuple(res))
        si, so = abi.SphIn(), abi.SphOut()
        si.vel_pred, si.vel_stride = addr(cols["vel_pred"]), 24
        si.hsml, si.hsml_stride = addr(res["hsml"]), 8
        si.des_num_ngb, si.max_num_ngb_deviation, si.min_gas_hsml = des_num_ngb, max_num_ngb_deviation, min_gas_hsml
        si.on_device = int(on_device)
        _set_columns(so, {k: res[k] for k in abi.SPH_OUT_NAMES}, addr)
        rounds, ms = C.c_int32(0), C.c_double(0)
        self._check(lib().ngravs_sph_density(self._h, C.byref(si), C.byref(so), C.byref(rounds), C.byref(ms)), "ngravs_sph_density")
        res["max_rounds"], res["kernel_ms"] = int(rounds.value), float(ms.value)
        return res

    def sph_hsml_guess(self, des_num_ngb, hsml=None, only_unset=False):
        """the first guess of the smoothing lengths, setup_smoothinglengths() of the reference for one task (init.c:229-247), from
        the built tree.  Returns the hsml column over all rows of the last hand-over: the guess in every type-0 row (only_unset:
        in those whose given value is not > 0), what `hsml` held in the others -- NaN when nothing was passed.  A numpy array, or
        a torch tensor on the device (float64, contiguous), is copied, not written."""
        on_device = hsml is not None and not isinstance(hsml, np.ndarray) and hasattr(hsml, "data_ptr")
        if on_device:
            import torch
            assert hsml.dtype == torch.float64 and hsml.is_contiguous()
            res = hsml.clone()
            torch.cuda.synchronize()
            addr = res.data_ptr()
        else:
            res = np.full(self.n, np.nan) if hsml is None else np.array(hsml, dtype=np.float64)
            addr = res.ctypes.data
        assert tuple(res.shape) == (self.n,)
        ms = C.c_double(0)
        self._check(lib().ngravs_sph_hsml_guess(self._h, float(des_num_ngb), addr, 8, int(bool(only_unset)), int(on_device), C.byref(ms)),
                    "ngravs_sph_hsml_guess")
        self.last_hsml_guess_ms = float(ms.value)
        return res

    def sph_hydro(self, vel, hsml, density, pressure, dhsml_factor, div_vel, curl_vel, *, art_bulk_visc_const, timestep=None,
                  timebase_interval=0.0, gamma=5.0 / 3, viscosity_limiter=True, comoving=None, out=None):
        """hydro_force() of the reference for one task (hydra.c:50-346): vel = SphP[].VelPred[N,3]; hsml, density, pressure,
        dhsml_factor, div_vel, curl_vel [N] as density() and the pressure line left them; timestep = Ti_endstep - Ti_begstep [N]
        int32 or None (all 0); one row per particle of the last hand-over.  Every type-0 row is read (all gas particles are
        sources), only rows of active type-0 particles are written.  comoving: None, or hydro_factors(...).  numpy arrays, or
        torch tensors on the device (float64 / int32, contiguous: no copy through the host).  Returns a dict: hydro_accel [N,3],
        dt_entropy, max_signal_vel (rows that are no targets: 0 -- or what `out`, a dict of arrays of the same kind, held),
        kernel_ms."""
        on_device = _is_device(vel)
        ins = dict(vel_pred=vel, hsml=hsml, density=density, pressure=pressure, dhsml_factor=dhsml_factor, div_vel=div_vel,
                   curl_vel=curl_vel, timestep=timestep)
        res = _results(abi.HYDRO_OUT_NAMES, self._rows, out, vel, on_device)
        cols, addr = _columns(dict(ins, **res), {k: self._rows(k) for k in list(ins) + list(res)}, on_device, int_keys=("timestep",),
                              own=tuple(res))
        hi, ho = abi.HydroIn(), abi.HydroOut()
        _set_columns(hi, {k: cols[k] for k in ins}, addr)
        _hydro_switches(hi, art_bulk_visc_const, timebase_interval, gamma, viscosity_limiter, comoving, on_device)
        _set_columns(ho, res, addr)
        ms = C.c_double(0)
        self._check(lib().ngravs_sph_hydro(self._h, C.byref(hi), C.byref(ho), C.byref(ms)), "ngravs_sph_hydro")
        res["kernel_ms"] = float(ms.value)
        return res

    def sph_accelerations(self, vel, entropy, hsml, density, pressure, dhsml_factor, div_vel, curl_vel, *, dt_entropy=None,
                          ti_begstep=None, ti_endstep=None, ti_current=0, timebase_interval=0.0, des_num_ngb, max_num_ngb_deviation,
                          min_gas_hsml=0.0, art_bulk_visc_const, gamma=5.0 / 3, viscosity_limiter=True, comoving=None, out=None):
        """The gas side of compute_accelerations() for one task in one call that stays on the device: density() with its pressure
        line (density.c:305-308), force_update_hmax(), hydro_force().  vel = SphP[].VelPred[N,3], entropy = SphP[].Entropy [N],
        dt_entropy = SphP[].DtEntropy of the step before or None (0), ti_begstep / ti_endstep int32 [N] or both None (dt_entr and
        every timestep 0); one row per particle of the last hand-over.  hsml, density, pressure, dhsml_factor, div_vel, curl_vel
        [N] are SphP[] as the reference holds it and are UPDATED IN PLACE: read for gas rows that are no targets, overwritten for
        the targets (a target's hsml is its starting guess).  numpy float64 C-contiguous arrays, or torch tensors on the device
        (float64 / int32, contiguous: no copy through the host).  comoving: None, or hydro_factors(...).  Returns a dict: num_ngb,
        hydro_accel [N,3], dt_entropy_out, max_signal_vel (rows that are no targets: 0 -- or what `out`, a dict of arrays of the
        same kind, held), max_rounds, kernel_ms (density walk, pressure line + hydro sources + hmax, hydro walk)."""
        on_device = _is_device(vel)
        ins = dict(vel_pred=vel, entropy=entropy, dt_entropy=dt_entropy, ti_begstep=ti_begstep, ti_endstep=ti_endstep)
        inout = dict(hsml=hsml, density=density, pressure=pressure, dhsml_factor=dhsml_factor, div_vel=div_vel, curl_vel=curl_vel)
        res = _results(abi.GAS_OUT_NAMES, self._rows, out, vel, on_device)
        # (the in/out columns are written through, as the results are: the caller's own arrays, never converted copies)
        cols, addr = _columns(dict(ins, **inout, **res), {k: self._rows(k) for k in list(ins) + list(inout) + list(res)}, on_device,
                              int_keys=("ti_begstep", "ti_endstep"), own=tuple(inout) + tuple(res))
        gi, go = abi.GasIn(), abi.GasOut()
        _set_columns(gi, {k: cols[k] for k in list(ins) + list(inout)}, addr)
        gi.des_num_ngb, gi.max_num_ngb_deviation, gi.min_gas_hsml = float(des_num_ngb), float(max_num_ngb_deviation), float(min_gas_hsml)
        gi.ti_current = int(ti_current)
        _hydro_switches(gi, art_bulk_visc_const, timebase_interval, gamma, viscosity_limiter, comoving, on_device)
        _set_columns(go, res, addr)
        rounds, ms = C.c_int32(0), (C.c_double * 3)()
        self._check(lib().ngravs_sph_accelerations(self._h, C.byref(gi), C.byref(go), C.byref(rounds), ms), "ngravs_sph_accelerations")
        res["max_rounds"], res["kernel_ms"] = int(rounds.value), [float(x) for x in ms]
        return res

    def sph_density_sums(self, vel, tpos, tvel, th):
        """density_evaluate(j, 1) of the reference (density.c:231-284): ONE round of the density sums over this engine's own gas
        for targets that need not be its particles.  vel = SphP[].VelPred[N,3] of the own rows; tpos, tvel [nt,3] and th [nt] the
        targets' positions, velocities and trial smoothing lengths, in any order.  numpy arrays, or torch tensors on the device.
        Returns sums [nt,7] (abi.SPH_SUM_NAMES: rho, the weighted neighbour number, dhsmlrho, div, rot[3]), RAW: add the sums of
        all engines, then sph_density_update()."""
        on_device = _is_device(vel)
        nt = int(tpos.shape[0])
        cols, addr = _columns(dict(vel=vel, pos=tpos, tvel=tvel, hsml=th), dict(vel=(self.n, 3), pos=(nt, 3), tvel=(nt, 3), hsml=(nt,)),
                              on_device)
        tg = abi.SphTargets()
        _set_columns(tg, dict(pos=cols["pos"], vel=cols["tvel"], hsml=cols["hsml"]), addr)
        sums = _zeros((nt, 7), vel, on_device)
        ms = C.c_double(0)
        self._check(lib().ngravs_sph_density_sums(self._h, addr(cols["vel"]), 24, C.byref(tg), nt, addr(sums), int(on_device), C.byref(ms)),
                    "ngravs_sph_density_sums")
        self.last_sums_ms = float(ms.value)
        return sums

    def sph_hydro_sums(self, vel, hsml, density, pressure, dhsml_factor, div_vel, curl_vel, targets, *, art_bulk_visc_const, timestep=None,
                       timebase_interval=0.0, gamma=5.0 / 3, viscosity_limiter=True, comoving=None):
        """hydro_evaluate(j, 1) of the reference (hydra.c:232-287): the hydro sums over this engine's own gas for targets that
        need not be its particles.  vel ... curl_vel, timestep: the own rows' columns as for sph_hydro (every own type-0 row is a
        source).  targets: a dict of the reference's hydrodata_in -- pos, vel [nt,3], hsml, mass, density, pressure, dhsml_factor,
        f1 [nt] and optionally timestep (int32 [nt]); sph_split.hydro_targets() builds it.  numpy arrays, or torch tensors on the
        device.  Returns sums [nt,5] (abi.HYDRO_SUM_NAMES): acc[3], dt_entropy BEFORE hydra.c:320, max_signal_vel."""
        on_device = _is_device(vel)
        n = self.n
        own = dict(vel_pred=vel, hsml=hsml, density=density, pressure=pressure, dhsml_factor=dhsml_factor, div_vel=div_vel,
                   curl_vel=curl_vel, timestep=timestep)
        own, addr = _columns(own, {k: (n, 3) if k == "vel_pred" else (n,) for k in own}, on_device, int_keys=("timestep",))
        nt = int(targets["pos"].shape[0])
        tcols = {k: targets.get(k) for k in abi.HYDRO_TARGET_NAMES}
        tcols, _ = _columns(tcols, {k: (nt, 3) if k in ("pos", "vel") else (nt,) for k in tcols}, on_device, int_keys=("timestep",))
        hi, tg = abi.HydroIn(), abi.HydroTargets()
        _set_columns(hi, own, addr)
        _set_columns(tg, tcols, addr)
        _hydro_switches(hi, art_bulk_visc_const, timebase_interval, gamma, viscosity_limiter, comoving, on_device)
        sums = _zeros((nt, 5), vel, on_device)
        ms = C.c_double(0)
        self._check(lib().ngravs_sph_hydro_sums(self._h, C.byref(hi), C.byref(tg), nt, addr(sums), int(on_device), C.byref(ms)),
                    "ngravs_sph_hydro_sums")
        self.last_sums_ms = float(ms.value)
        return sums

    def stats(self):
        s = Stats()
        self._check(lib().ngravs_get_stats(self._h, C.byref(s)), "ngravs_get_stats")
        return s

    def domain(self):
        d = np.zeros(8)
        self._check(lib().ngravs_get_domain(self._h, d.ctypes.data), "ngravs_get_domain")
        return d

    def keys(self):
        k = np.zeros(self.n, dtype=np.int64)
        self._check(lib().ngravs_get_keys(self._h, k.ctypes.data, 0), "ngravs_get_keys")
        return k

    def order(self):
        o = np.zeros(self.n, dtype=np.int32)
        self._check(lib().ngravs_get_order(self._h, o.ctypes.data, 0), "ngravs_get_order")
        return o

    def shard(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(lib().ngravs_get_shard(self._h, C.byref(a), C.byref(b)), "ngravs_get_shard")
        return int(a.value), int(b.value)

    def peano_keys(self, pos, corner, fac, bits=18):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        corner = np.ascontiguousarray(corner, dtype=np.float64)
        out = np.zeros(len(pos), dtype=np.int64)
        self._check(lib().ngravs_peano_keys(self._h, pos.ctypes.data, len(pos), corner.ctypes.data, float(fac), bits,
                                            out.ctypes.data), "ngravs_peano_keys")
        return out

    def direct_sum_targets(self, pos, ptype, mass=None):
        """partial direct sums of explicit targets over this task's OWN particles (distributed gravity_forcetest): add over tasks"""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        ptype = np.ascontiguousarray(ptype, dtype=np.int32)
        mass = np.ascontiguousarray(mass, dtype=np.float64) if mass is not None else None
        out = np.zeros((len(pos), 3))
        self._check(lib().ngravs_direct_sum_targets(self._h, pos.ctypes.data, _ptr(mass), ptype.ctypes.data, len(pos), out.ctypes.data),
                    "ngravs_direct_sum_targets")
        return out

    @staticmethod
    def _grav_targets(pos, ptype, old_acc=None, mass=None):
        """(abi.GravTargets, nt, on_device, the arrays it points to) for target records given as numpy arrays or torch tensors on
        the device.  Needs no device: a pos that is not floating point [nt,3] or a ptype that is not integer [nt] is a ValueError."""
        on_device = _is_device(pos)
        if not on_device:
            pos, ptype = np.asarray(pos), np.asarray(ptype)
        if len(pos.shape) != 2 or pos.shape[1] != 3 or not ("float" in str(pos.dtype)):
            raise ValueError("pos must be a floating-point array of shape [nt, 3], not %s %s" % (pos.dtype, tuple(pos.shape)))
        nt = int(pos.shape[0])
        if tuple(ptype.shape) != (nt,) or not ("int" in str(ptype.dtype)):
            raise ValueError("ptype must be an integer array of shape [%d], not %s %s" % (nt, ptype.dtype, tuple(ptype.shape)))
        if on_device:
            import torch
            ptype = ptype.to(torch.int32)   # (the other columns must be float64 as they are: _columns)
        cols, addr = _columns(dict(pos=pos, type=ptype, old_acc=old_acc, mass=mass), dict(pos=(nt, 3), type=(nt,), old_acc=(nt,), mass=(nt,)),
                              on_device, int_keys=("type",))
        tg = abi.GravTargets()
        _set_columns(tg, cols, addr)
        tg.on_device = int(on_device)
        return tg, nt, on_device, cols

    def gravity_tree_targets(self, pos, ptype, old_acc=None, mass=None, want_nint=False):
        """The tree force of this engine's particles at targets that need not be its particles (the reference's walk for imported
        particles, force_treeevaluate(j, 1) / _shortrange(j, 1), gravtree.c:133-285): pos [nt,3], ptype [nt], old_acc [nt] or None
        (0: the relative criterion then opens every node), mass [nt] or None (1; only the BAM laws read it), in any order.  Always
        the strict walk, with the engine's current opening criterion; TreePM engines give the short-range force (add pm_targets()).
        numpy arrays, or torch tensors on the device.  Returns acc [nt,3] (x G), or (acc, nint) with the interaction counts.  The
        engine's own accelerations are not touched."""
        tg, nt, on_device, keep = self._grav_targets(pos, ptype, old_acc, mass)
        acc = _zeros((nt, 3), pos, on_device)
        nint = _zeros(nt, pos, on_device, np.int32)
        ms = C.c_double(0)
        if nt > 0:
            addr = (lambda a: a.data_ptr()) if on_device else (lambda a: a.ctypes.data)
            self._check(lib().ngravs_gravity_tree_targets(self._h, C.byref(tg), nt, addr(acc), addr(nint), C.byref(ms)),
                        "ngravs_gravity_tree_targets")
        self.last_targets_ms = float(ms.value)
        del keep
        return (acc, nint) if want_nint else acc

    def pm_targets(self, pos, ptype):
        """GravPM of the last PM step's mesh at targets that need not be this engine's particles: pos [nt,3] inside [0, BoxSize],
        ptype [nt]; numpy arrays, or torch tensors on the device.  Returns grav_pm [nt,3], G included.  The mesh stays valid across
        steps without PM."""
        tg, nt, on_device, keep = self._grav_targets(pos, ptype)
        pm = _zeros((nt, 3), pos, on_device)
        if nt > 0:
            self._check(lib().ngravs_pm_targets(self._h, C.byref(tg), nt, pm.data_ptr() if on_device else pm.ctypes.data), "ngravs_pm_targets")
        del keep
        return pm

    # -- gravitational potentials: compute_potential() (potential.c:22-345) ----------------------------------------------------
    def compute_potential(self, par=None, into=None, want_nint=False):
        """P[].Potential of ALL rows of the last hand-over, in the caller's order, from the built tree (and, with a mesh, a mesh
        potential at the current positions): walk, self term, G, mesh part, cosmological term (ngravs_compute_potential).  par:
        abi.make_time_params(...) for a comoving run or one with OmegaLambda, else None.  into: None (a fresh numpy array), or the
        float64 [n] column to write, a C-contiguous numpy array or a contiguous torch tensor on the device.  Returns the column,
        or (column, nint) with the int32 interaction counts of the walk.  Accelerations, GravPM and costs are not touched; with a
        mesh pm_targets() is refused afterwards until the next PM step."""
        on_device = into is not None and _is_device(into)
        if into is not None:
            if "float64" not in str(into.dtype) or len(into.shape) != 1:
                raise ValueError("into must be a float64 array of shape [n], not %s %s" % (into.dtype, tuple(into.shape)))
            if not (into.is_contiguous() if on_device else into.flags.c_contiguous):
                raise ValueError("into must be contiguous: it is written through")
            if int(into.shape[0]) != self.n:
                raise ValueError("into has %d rows, the engine %d" % (int(into.shape[0]), self.n))
        pot = into if into is not None else np.zeros(self.n)
        nint = _zeros(self.n, into, on_device, np.int32) if want_nint else None
        if on_device:
            import torch
            torch.cuda.synchronize()   # the library works on a stream of its own
        addr = (lambda a: None if a is None else a.data_ptr()) if on_device else _ptr
        self._check(lib().ngravs_compute_potential(self._h, C.byref(par) if par is not None else None, addr(pot), 8, int(on_device),
                                                   addr(nint)), "ngravs_compute_potential")
        return (pot, nint) if want_nint else pot

    def potential_targets(self, pos, ptype, old_acc=None, mass=None, want_nint=False):
        """The potential of this engine's particles at targets that need not be its particles: the records of
        gravity_tree_targets(), in any order.  Returns pot [nt] = the potential walk x G, plus the mesh part with a mesh (that of
        the last compute_potential(), which must have been called since the last PM step and hand-over); no self term and no
        cosmological term, so the potentials of a set split over engines add up.  Or (pot, nint)."""
        tg, nt, on_device, keep = self._grav_targets(pos, ptype, old_acc, mass)
        pot = _zeros(nt, pos, on_device)
        nint = _zeros(nt, pos, on_device, np.int32)
        if nt > 0:
            addr = (lambda a: a.data_ptr()) if on_device else (lambda a: a.ctypes.data)
            self._check(lib().ngravs_potential_targets(self._h, C.byref(tg), nt, addr(pot), addr(nint)), "ngravs_potential_targets")
        del keep
        return (pot, nint) if want_nint else pot

    def lattice_potential_table(self, t, s):
        """the lattice potential table of the species pair (t, s) as the periodic tree-only potential walk reads it: float64
        [65, 65, 65], sign(law) ewald_psi(i / 128, j / 128, k / 128) / BoxSize, the origin sign(law) 2.8372975 / BoxSize"""
        for k in (t, s):
            if int(k) != k or not 0 <= int(k) < abi.MAX_GRAVS:
                raise ValueError("species %r is outside 0..%d" % (k, abi.MAX_GRAVS - 1))
        out = np.zeros((65, 65, 65))
        self._check(lib().ngravs_lattice_potential_table(self._h, int(t), int(s), out.ctypes.data), "ngravs_lattice_potential_table")
        return out

    def last_potential_ms(self):
        """device milliseconds of the walk kernel of the last compute_potential()"""
        ms = C.c_double(0)
        self._check(lib().ngravs_last_potential_ms(self._h, C.byref(ms)), "ngravs_last_potential_ms")
        return float(ms.value)

    # -- time integration: the stations of run.c:32-65 around the forces ------------------------------------------------------
    @staticmethod
    def _time_cols(cols):
        """abi.TimeCols for a dict of columns by the names of abi.TIME_COL_NAMES: numpy arrays (C-contiguous, float64 / int32:
        they are written through) or contiguous torch tensors on the device, all of one kind; [n,3] for the vectors, [n] else"""
        given = {k: a for k, a in cols.items() if a is not None}
        unknown = set(given) - set(abi.TIME_COL_NAMES)
        if unknown:
            raise TypeError("unknown columns %s" % sorted(unknown))
        first = next(iter(given.values()))
        on_device, n = _is_device(first), int(first.shape[0])
        shapes = {k: (n, 3) if k in abi.TIME_VEC_COLS else (n,) for k in given}
        chk, addr = _columns(given, shapes, on_device, int_keys=abi.TIME_INT_COLS, own=tuple(given))
        tc = abi.TimeCols()
        _set_columns(tc, chk, addr)
        tc.n, tc.on_device = n, int(on_device)
        return tc, chk

    def time_tables(self, par, rule=0):
        return time_tables(par, rule)

    def asmth(self):
        """All.Asmth[0] of the configuration (pm_periodic.c:59), 0 without a mesh"""
        if self.cfg.pmgrid <= 0:
            return 0.0
        return self.cfg.asmth if self.cfg.asmth > 0 else abi.ASMTH * self.cfg.box_size / self.cfg.pmgrid

    def next_sync_point(self, ti_endstep, pm_ti_endstep=None):
        """run.c:161-191: (ti_next, full_step, n_active) from the Ti_endstep column (int32 [n]; numpy or a device tensor);
        pm_ti_endstep: All.PM_Ti_endstep, or None without a mesh"""
        tc, keep = self._time_cols(dict(ti_endstep=ti_endstep))
        out = abi.SyncPoint()
        self._check(lib().ngravs_next_sync_point(self._h, C.byref(tc), -1 if pm_ti_endstep is None else int(pm_ti_endstep), C.byref(out)),
                    "ngravs_next_sync_point")
        return int(out.ti_next), bool(out.full_step), int(out.n_active)

    def move_particles(self, cols, par, time0, time1, wrap=False):
        """move_particles(time0, time1) of the reference (predict.c:31-76) on the caller's columns, IN PLACE: cols is a dict by
        the names of abi.TIME_COL_NAMES -- type, pos, vel, and for gas vel_pred, grav_accel, grav_pm (with a mesh), hydro_accel,
        density, hsml, pressure, div_vel, entropy, dt_entropy, ti_begstep, ti_endstep.  wrap: do_box_wrapping() afterwards."""
        tc, keep = self._time_cols(cols)
        self._check(lib().ngravs_move_particles(self._h, C.byref(tc), C.byref(par), int(time0), int(time1), int(bool(wrap))),
                    "ngravs_move_particles")

    def displacement_sums(self, ptype, vel, mass):
        """the 18 local sums of find_dt_displacement_constraint (timestep.c:606-612): per type the sum of |v|^2, the smallest
        mass, the count"""
        tc, keep = self._time_cols(dict(type=ptype, vel=vel, mass=mass))
        sums = np.zeros(18)
        self._check(lib().ngravs_displacement_sums(self._h, C.byref(tc), sums.ctypes.data), "ngravs_displacement_sums")
        return sums

    def dt_displacement(self, par, sums, time):
        """the displacement constraint from the (all-reduced) sums, with the configuration's G and Asmth"""
        return dt_displacement(par, sums, self.cfg.G, self.asmth(), time)

    def advance_and_find_timesteps(self, cols, par, ti_current, dt_displacement, pm_ti=None):
        """advance_and_find_timesteps() of the reference (timestep.c:24-413) on the caller's columns, IN PLACE, for the rows with
        ti_endstep == ti_current: cols holds type, vel, ti_begstep, ti_endstep, grav_accel, grav_pm (with a mesh), and for gas
        vel_pred, hydro_accel, entropy, dt_entropy, density, hsml, max_signal_vel.  pm_ti: [PM_Ti_begstep, PM_Ti_endstep] with a
        mesh.  Returns (rows advanced, the new pm_ti or None)."""
        tc, keep = self._time_cols(cols)
        pm = (C.c_int32 * 2)(*[int(x) for x in pm_ti]) if pm_ti is not None else None
        kicked = C.c_int64(0)
        self._check(lib().ngravs_advance_and_find_timesteps(self._h, C.byref(tc), C.byref(par), int(ti_current), float(dt_displacement), pm,
                                                            C.byref(kicked)), "ngravs_advance_and_find_timesteps")
        return int(kicked.value), (None if pm is None else [int(pm[0]), int(pm[1])])

    def global_sums(self, cols, par, ti_current, pm_ti=None, potential=None):
        """the task's 78 sums of compute_global_quantities_of_system() (global.c:52-114) at All.Ti_Current = ti_current: float64
        [78], [13 * type + k] with k = mass, kinetic, internal and potential energy, m vel [3], m pos x vel [3], m pos [3].  cols
        holds type, pos, vel, mass, ti_begstep, ti_endstep, grav_accel, grav_pm (with a mesh), and for gas hydro_accel, entropy,
        dt_entropy, density; nothing is written.  pm_ti: [PM_Ti_begstep, PM_Ti_endstep] with a mesh.  potential: None (EnergyPot
        is 0 then), or P[].Potential, float64 [n] of the kind of the columns.  A host with several tasks adds the sums of its
        tasks before global_finish()."""
        tc, keep = self._time_cols(cols)
        pot = None
        if potential is not None:
            pcol, addr = _columns(dict(potential=potential), dict(potential=(int(tc.n),)), bool(tc.on_device))
            pot = addr(pcol["potential"])
        pm = (C.c_int32 * 2)(*[int(x) for x in pm_ti]) if pm_ti is not None else None
        sums = np.zeros(abi.GLOBAL_NSUMS)
        self._check(lib().ngravs_global_sums(self._h, C.byref(tc), C.byref(par), int(ti_current), pm, pot, 8, sums.ctypes.data),
                    "ngravs_global_sums")
        return sums

    def global_quantities(self, cols, par, ti_current, pm_ti=None, potential=None):
        """compute_global_quantities_of_system() for one task: global_finish(global_sums(...)), an abi.SysState"""
        return global_finish(self.global_sums(cols, par, ti_current, pm_ti, potential))

    # -- snapshot files: savepositions() (io.c:33-989) ---------------------------------------------------------------------------
    def _snap_cols(self, cols):
        """cols as the time calls take them, or a ready abi.TimeCols (any strides: an interleaved P[])"""
        if isinstance(cols, abi.TimeCols):
            return cols, None
        return self._time_cols(cols)

    def _snapshot(self, tc, ti_current, pm_ti, mass_table, ids, potential, box_size=None, hubble_param=0.0):
        """abi.Snapshot; ids / potential: an array of the kind of the columns (int32 / float64 [n]), or (address, stride)"""
        s = abi.Snapshot()
        keep = []
        s.ti_current = int(ti_current)
        if pm_ti is not None:
            pm = (C.c_int32 * 2)(*[int(x) for x in pm_ti])
            keep.append(pm)
            s.pm_ti = C.addressof(pm)
        s.mass_table = (C.c_double * 6)(*([0.0] * 6 if mass_table is None else [float(x) for x in mass_table]))
        for name, col, key in (("ids", ids, "type"), ("potential", potential, "mass")):
            if col is None:
                continue
            if isinstance(col, tuple):
                a, stride = col
            else:
                chk, addr = _columns({name: col}, {name: (int(tc.n),)}, bool(tc.on_device), int_keys=("ids",))
                keep.append(chk)
                a, stride = addr(chk[name]), 4 if name == "ids" else 8
            setattr(s, name, a)
            setattr(s, name + "_stride", stride)
        s.box_size = float(self.cfg.box_size if box_size is None else box_size)
        s.hubble_param = float(hubble_param)
        s._keep = keep
        return s

    def snapshot_plan(self, cols):
        """The file order of io.c for the type column (cols: a dict with "type", or an abi.TimeCols): a stable partition of the
        rows by type, kept in the engine until the next plan.  Returns npart, int64 [6]."""
        tc, keep = self._snap_cols(cols if isinstance(cols, (dict, abi.TimeCols)) else dict(type=cols))
        npart = np.zeros(6, dtype=np.int64)
        self._check(lib().ngravs_snapshot_plan(self._h, C.byref(tc), npart.ctypes.data), "ngravs_snapshot_plan")
        return npart

    def snapshot_block_count(self, block, mass_table=None):
        """get_particles_in_block (io.c:465-523) for the plan: (elements, bytes per element)"""
        s = abi.Snapshot()
        s.mass_table = (C.c_double * 6)(*([0.0] * 6 if mass_table is None else [float(x) for x in mass_table]))
        cnt, bpe = C.c_int64(0), C.c_int32(0)
        self._check(lib().ngravs_snapshot_block_count(self._h, C.byref(s), int(block), C.byref(cnt), C.byref(bpe)), "ngravs_snapshot_block_count")
        return int(cnt.value), int(bpe.value)

    def snapshot_block(self, block, cols, par, ti_current, pm_ti=None, mass_table=None, ids=None, potential=None, first=0, count=None,
                       out=None, device_out=None):
        """The elements [first, first + count) of a block (abi.SNAP_*) of the planned file order as they lie on disk: float32
        [count] or [count, 3], int32 for ID.  Returns a numpy array, or a device tensor when the columns are device tensors
        (device_out overrides); out: written through instead."""
        tc, keep = self._snap_cols(cols)
        s = self._snapshot(tc, ti_current, pm_ti, mass_table, ids, potential)
        if count is None:
            count = self.snapshot_block_count(block, mass_table)[0] - int(first)
        on_dev = bool(tc.on_device) if device_out is None else bool(device_out)
        shape = (int(count), 3) if block in abi.SNAP_VECTOR_BLOCKS else (int(count),)
        if out is None:
            if on_dev:
                import torch
                out = torch.zeros(shape, dtype=torch.int32 if block == abi.SNAP_ID else torch.float32, device="cuda")
                torch.cuda.synchronize()
            else:
                out = np.zeros(shape, dtype=np.int32 if block == abi.SNAP_ID else np.float32)
        addr = out.data_ptr() if _is_device(out) else out.ctypes.data
        self._check(lib().ngravs_snapshot_block(self._h, C.byref(tc), C.byref(par), C.byref(s), int(block), int(first), int(count), addr,
                                                int(_is_device(out))), "ngravs_snapshot_block")
        return out

    def snapshot_header(self, par, npart, time, mass_table=None, npart_total=None, num_files=1, hubble_param=0.0, box_size=None):
        return snapshot_header(par, npart, time, mass_table, npart_total, num_files, hubble_param,
                               self.cfg.box_size if box_size is None else box_size)

    def write_snapshot(self, path, cols, par, ti_current, pm_ti=None, mass_table=None, ids=None, potential=None, blocks_mask=abi.SNAP_ALWAYS,
                       snap_format=1, buffer_bytes=0, hubble_param=0.0, box_size=None):
        """savepositions() for one task and one file (io.c:33-989): plan, header and every present block with elements, converted
        and grouped by type on the device, framed on the host.  cols: the columns of the time calls (dict, or abi.TimeCols); ids:
        P[].ID (int32 [n]); potential: P[].Potential for the POT block; blocks_mask: abi.snap_mask("ACCE", ...) for the
        reference's OUTPUT* switches; snap_format 1 or 2; buffer_bytes: the chunk that crosses to the host at a time (0: 64 MiB)."""
        tc, keep = self._snap_cols(cols)
        s = self._snapshot(tc, ti_current, pm_ti, mass_table, ids, potential, box_size, hubble_param)
        self._check(lib().ngravs_snapshot_write(self._h, C.byref(tc), C.byref(par), C.byref(s), int(blocks_mask), int(snap_format), int(buffer_bytes),
                                                os.fsencode(path)), "ngravs_snapshot_write")

    def direct_sum(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.zeros((len(idx), 3))
        self._check(lib().ngravs_direct_sum(self._h, idx.ctypes.data, len(idx), out.ctypes.data), "ngravs_direct_sum")
        return out

from . import sph_split  # noqa: E402,F401  (uses NgravsError and sph_density_update above)
from . import timeline  # noqa: E402,F401
from . import snapshot  # noqa: E402,F401
