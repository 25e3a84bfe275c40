"""ctypes binding of libpeaksegdisk_hip.so (the C ABI declared in include/peaksegdisk_hip.h).

The library is the only solver: importing this module fails loudly when it has not been
built (`python -c "import __graft_entry__ as g; g.build()"`), and every dynamic program
fails with ERROR_NO_HIP_DEVICE when no MI355X is visible.  There is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpeaksegdisk_hip.so")

ERROR_NO_HIP_DEVICE = 12
ERROR_DEVICE_SOLVER = 13
ERROR_DEVICE_MEMORY = 14
ERROR_DENSE_ARGUMENTS = 17
ERROR_READS_ARGUMENTS = 18
ERROR_LABEL_ARGUMENTS = 19
ERROR_FEATURE_ARGUMENTS = 20
ERROR_FIT_ARGUMENTS = 21
ERROR_REGION_ARGUMENTS = 22
ERROR_HELDOUT_ARGUMENTS = 23
ERROR_STRAND_ARGUMENTS = 24
ERROR_DEDUP_ARGUMENTS = 25


class PsdResult(ctypes.Structure):
    _fields_ = [
        ("status", ctypes.c_int),
        ("kernel_status", ctypes.c_int),
        ("n_segments", ctypes.c_int),
        ("n_peaks", ctypes.c_int),
        ("n_equality_constraints", ctypes.c_int),
        ("max_intervals", ctypes.c_int),
        ("total_intervals", ctypes.c_ulonglong),
        ("best_cost", ctypes.c_double),
        ("n_serial_env", ctypes.c_int),
        ("step_reached", ctypes.c_int),
        ("spill_steps", ctypes.c_int),
    ]


class PsdSearchRow(ctypes.Structure):
    _fields_ = [
        ("penalty_str", ctypes.c_char * 40),
        ("penalty", ctypes.c_double),
        ("total_loss", ctypes.c_double),
        ("peaks", ctypes.c_int),
        ("segments", ctypes.c_int),
        ("bases", ctypes.c_int),
        ("iteration", ctypes.c_int),
        ("under_peaks", ctypes.c_int),
        ("over_peaks", ctypes.c_int),
        ("cached", ctypes.c_int),
    ]


ERROR_SEARCH_ARGUMENTS = 15
ERROR_SEARCH_TOO_MANY_PEAKS = 16
SEARCH_NA = -2 ** 31


def declare(lib):
    """Attach argtypes/restypes for every symbol of include/peaksegdisk_hip.h."""
    c = ctypes
    lib.PeakSegFPOP_disk.argtypes = [c.c_char_p, c.c_char_p, c.c_char_p]
    lib.PeakSegFPOP_disk.restype = c.c_int
    lib.PeakSegFPOP_disk_batch.argtypes = [
        c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_char_p), c.POINTER(c.c_char_p),
        c.POINTER(c.c_int)]
    lib.PeakSegFPOP_disk_batch.restype = c.c_int
    lib.PeakSegFPOP_status_message.argtypes = [
        c.c_int, c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p, c.c_size_t]
    lib.PeakSegFPOP_status_message.restype = c.c_char_p
    lib.peakseg_hip_set_print.argtypes = [c.c_void_p]
    lib.peakseg_hip_set_print.restype = None
    lib.peakseg_hip_device_count.argtypes = []
    lib.peakseg_hip_device_count.restype = c.c_int
    lib.peakseg_hip_last_error.argtypes = []
    lib.peakseg_hip_last_error.restype = c.c_char_p
    lib.peakseg_hip_problem_set_create.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_double), c.c_ulonglong,
        c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_create.restype = c.c_int
    lib.peakseg_hip_problem_set_solve.argtypes = [
        c.c_void_p, c.POINTER(c.c_float), c.POINTER(c.c_float)]
    lib.peakseg_hip_problem_set_solve.restype = c.c_int
    lib.peakseg_hip_problem_set_result.argtypes = [c.c_void_p, c.c_int, c.POINTER(PsdResult)]
    lib.peakseg_hip_problem_set_result.restype = c.c_int
    lib.peakseg_hip_problem_set_segments.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_segments.restype = c.c_int
    lib.peakseg_hip_problem_set_export_db.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_char_p]
    lib.peakseg_hip_problem_set_export_db.restype = c.c_int
    lib.peakseg_hip_problem_set_bytes.argtypes = [c.c_void_p]
    lib.peakseg_hip_problem_set_bytes.restype = c.c_ulonglong
    lib.peakseg_hip_problem_set_kernel_build.argtypes = [c.c_void_p]
    lib.peakseg_hip_problem_set_kernel_build.restype = c.c_char_p
    lib.peakseg_hip_problem_set_destroy.argtypes = [c.c_void_p]
    lib.peakseg_hip_problem_set_destroy.restype = None
    lib.peakseg_hip_parse_probe.argtypes = [c.c_char_p, c.c_int, c.POINTER(c.c_int),
                                            c.POINTER(c.c_ulonglong)]
    lib.peakseg_hip_parse_probe.restype = c.c_int
    lib.peakseg_hip_problem_set_profile.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    lib.peakseg_hip_problem_set_profile.restype = c.c_int
    lib.peakseg_hip_math_probe.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_math_probe.restype = c.c_int
    lib.peakseg_hip_math_forms_probe.argtypes = [c.c_int] * 3 + [c.c_void_p] * 7
    lib.peakseg_hip_math_forms_probe.restype = c.c_int
    lib.PeakSegFPOP_dir_batch.argtypes = [
        c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_char_p), c.POINTER(c.c_int),
        c.POINTER(c.c_int)]
    lib.PeakSegFPOP_dir_batch.restype = c.c_int
    lib.PeakSegFPOP_sequential_search.argtypes = [
        c.c_char_p, c.c_int, c.c_int, c.c_int, c.POINTER(PsdSearchRow), c.POINTER(c.c_int),
        c.POINTER(c.c_int)]
    lib.PeakSegFPOP_sequential_search.restype = c.c_int
    lib.PeakSegFPOP_sequential_search_batch.argtypes = [
        c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_int), c.c_int, c.c_int,
        c.POINTER(PsdSearchRow), c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]
    lib.PeakSegFPOP_sequential_search_batch.restype = c.c_int
    lib.PeakSegFPOP_parallel_search.argtypes = [
        c.c_char_p, c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(PsdSearchRow),
        c.POINTER(c.c_int), c.POINTER(c.c_int)]
    lib.PeakSegFPOP_parallel_search.restype = c.c_int
    lib.PeakSegFPOP_parallel_search_batch.argtypes = [
        c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_int), c.c_int, c.c_int, c.c_int,
        c.POINTER(PsdSearchRow), c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]
    lib.PeakSegFPOP_parallel_search_batch.restype = c.c_int
    lib.peakseg_hip_problem_set_set_penalty.argtypes = [c.c_void_p, c.c_int, c.c_double]
    lib.peakseg_hip_problem_set_set_penalty.restype = c.c_int
    lib.peakseg_hip_problem_set_arena_bytes_used.argtypes = [c.c_void_p]
    lib.peakseg_hip_problem_set_arena_bytes_used.restype = c.c_ulonglong
    lib.peakseg_hip_problem_set_checkpoint_interval.argtypes = [c.c_void_p]
    lib.peakseg_hip_problem_set_checkpoint_interval.restype = c.c_int
    lib.peakseg_hip_paste_double.argtypes = [c.c_double, c.c_char_p, c.c_size_t]
    lib.peakseg_hip_paste_double.restype = c.c_int
    lib.peakseg_hip_problem_set_solve_stats.argtypes = [
        c.c_void_p, c.POINTER(c.c_int), c.POINTER(c.c_ulonglong)]
    lib.peakseg_hip_problem_set_solve_stats.restype = c.c_int
    lib.peakseg_hip_device_clock_khz.argtypes = [c.c_int]
    lib.peakseg_hip_device_clock_khz.restype = c.c_int
    lib.peakseg_hip_problem_set_park_stats.argtypes = [
        c.c_void_p, c.POINTER(c.c_int), c.POINTER(c.c_ulonglong)]
    lib.peakseg_hip_problem_set_park_stats.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_tables.argtypes = [
        c.c_void_p, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_tables.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_download.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_download.restype = c.c_int
    lib.peakseg_hip_problem_set_cycles.argtypes = [c.c_void_p, c.c_int]
    lib.peakseg_hip_problem_set_cycles.restype = c.c_longlong
    lib.peakseg_hip_measured_rates.argtypes = [c.POINTER(c.c_double), c.POINTER(c.c_double)]
    lib.peakseg_hip_measured_rates.restype = None
    lib.peakseg_hip_spin_limit.argtypes = []
    lib.peakseg_hip_spin_limit.restype = c.c_longlong
    lib.peakseg_hip_problem_set_max_spin.argtypes = [c.c_void_p, c.c_int]
    lib.peakseg_hip_problem_set_max_spin.restype = c.c_int
    lib.peakseg_hip_problem_set_loop_stats.argtypes = [c.c_void_p, c.c_int, c.POINTER(c.c_int)]
    lib.peakseg_hip_problem_set_loop_stats.restype = c.c_int
    lib.peakseg_hip_last_warning.argtypes = []
    lib.peakseg_hip_last_warning.restype = c.c_char_p
    lib.peakseg_hip_problem_set_arena_stats.argtypes = [
        c.c_void_p, c.POINTER(c.c_ulonglong), c.POINTER(c.c_int), c.POINTER(c.c_int)]
    lib.peakseg_hip_problem_set_arena_stats.restype = c.c_int
    lib.peakseg_hip_last_fanout.argtypes = [
        c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_double)]
    lib.peakseg_hip_last_fanout.restype = c.c_int
    lib.peakseg_hip_last_fanout_entries.argtypes = [c.c_int, c.POINTER(c.c_int)]
    lib.peakseg_hip_last_fanout_entries.restype = c.c_int
    lib.peakseg_hip_problem_set_create_dense.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.c_int,
        c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_double), c.c_ulonglong,
        c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_create_dense.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_segments.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_segments.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_segments_download.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_segments_download.restype = c.c_int
    lib.peakseg_hip_problem_set_loss.argtypes = [c.c_void_p, c.c_int, c.POINTER(c.c_double)]
    lib.peakseg_hip_problem_set_loss.restype = c.c_int
    lib.peakseg_hip_dense_encode_probe.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.c_int,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_dense_encode_probe.restype = c.c_int
    lib.peakseg_hip_dense_tile_bases.argtypes = []
    lib.peakseg_hip_dense_tile_bases.restype = c.c_int
    lib.peakseg_hip_dense_last_encode_ms.argtypes = [
        c.POINTER(c.c_float), c.POINTER(c.c_float), c.POINTER(c.c_float)]
    lib.peakseg_hip_dense_last_encode_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_segment_stats.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_segment_stats.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_segment_stats_download.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_segment_stats_download.restype = c.c_int
    lib.peakseg_hip_segment_stats_tile_runs.argtypes = []
    lib.peakseg_hip_segment_stats_tile_runs.restype = c.c_int
    lib.peakseg_hip_segment_stats_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_segment_stats_last_ms.restype = c.c_int
    reads = [c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p),
             c.POINTER(c.c_void_p), c.POINTER(c.c_void_p), c.c_int, c.POINTER(c.c_int),
             c.POINTER(c.c_int), c.c_int]
    lib.peakseg_hip_problem_set_create_reads.argtypes = reads + [
        c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_double), c.c_ulonglong, c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_create_reads.restype = c.c_int
    lib.peakseg_hip_reads_pileup_probe.argtypes = reads + [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_reads_pileup_probe.restype = c.c_int
    lib.peakseg_hip_reads_last_pileup_ms.argtypes = [c.POINTER(c.c_float), c.POINTER(c.c_float)]
    lib.peakseg_hip_reads_last_pileup_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_label_errors.argtypes = [
        c.c_void_p, c.c_void_p, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.POINTER(c.c_void_p), c.c_int, c.c_void_p, c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_label_errors.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_label_errors_download.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_label_errors_download.restype = c.c_int
    lib.peakseg_hip_label_errors_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_label_errors_last_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_coverage_stats.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_coverage_stats.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_coverage_stats_download.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_coverage_stats_download.restype = c.c_int
    lib.peakseg_hip_coverage_stats_tile_runs.argtypes = []
    lib.peakseg_hip_coverage_stats_tile_runs.restype = c.c_int
    lib.peakseg_hip_coverage_stats_max_ranks.argtypes = []
    lib.peakseg_hip_coverage_stats_max_ranks.restype = c.c_int
    lib.peakseg_hip_coverage_stats_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_coverage_stats_last_ms.restype = c.c_int
    lib.peakseg_hip_coverage_stats_last_passes.argtypes = [c.POINTER(c.c_int)]
    lib.peakseg_hip_coverage_stats_last_passes.restype = c.c_int
    lib.peakseg_hip_penalty_fit.argtypes = [
        c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int,
        c.c_void_p, c.c_double, c.c_double, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_void_p]
    lib.peakseg_hip_penalty_fit.restype = c.c_int
    lib.peakseg_hip_penalty_fit_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_penalty_fit_last_ms.restype = c.c_int
    lib.peakseg_hip_penalty_fit_max_features.argtypes = []
    lib.peakseg_hip_penalty_fit_max_features.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_region_stats.argtypes = [
        c.c_void_p, c.c_void_p, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.c_int, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_pack_region_stats.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_region_stats_download.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_problem_set_packed_region_stats_download.restype = c.c_int
    lib.peakseg_hip_region_stats_tile_runs.argtypes = []
    lib.peakseg_hip_region_stats_tile_runs.restype = c.c_int
    lib.peakseg_hip_region_stats_last_fold_grid.argtypes = []
    lib.peakseg_hip_region_stats_last_fold_grid.restype = c.c_longlong
    lib.peakseg_hip_region_stats_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_region_stats_last_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_peak_clusters.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p] + \
        [c.POINTER(c.c_void_p)] * 8
    lib.peakseg_hip_problem_set_pack_peak_clusters.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_peak_clusters_download.argtypes = [c.c_void_p] * 9
    lib.peakseg_hip_problem_set_packed_peak_clusters_download.restype = c.c_int
    lib.peakseg_hip_peak_clusters_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_peak_clusters_last_ms.restype = c.c_int
    lib.peakseg_hip_peak_clusters_probe.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.peakseg_hip_peak_clusters_probe.restype = c.c_longlong
    lib.peakseg_hip_problem_set_pack_joint_peaks.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_int, c.c_void_p, c.c_void_p] + [c.POINTER(c.c_void_p)] * 11
    lib.peakseg_hip_problem_set_pack_joint_peaks.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_joint_peaks_download.argtypes = [c.c_void_p] * 12
    lib.peakseg_hip_problem_set_packed_joint_peaks_download.restype = c.c_int
    lib.peakseg_hip_joint_peaks_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_joint_peaks_last_ms.restype = c.c_int
    lib.peakseg_hip_joint_path_max_penalties.argtypes = []
    lib.peakseg_hip_joint_path_max_penalties.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_joint_path.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p] + [c.POINTER(c.c_void_p)] * 11
    lib.peakseg_hip_problem_set_pack_joint_path.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_joint_path_download.argtypes = [c.c_void_p] * 12
    lib.peakseg_hip_problem_set_packed_joint_path_download.restype = c.c_int
    lib.peakseg_hip_joint_path_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_joint_path_last_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_joint_label_errors.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int] + \
        [c.POINTER(c.c_void_p)] * 5
    lib.peakseg_hip_problem_set_pack_joint_label_errors.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_joint_label_errors_download.argtypes = [c.c_void_p] * 6
    lib.peakseg_hip_problem_set_packed_joint_label_errors_download.restype = c.c_int
    lib.peakseg_hip_joint_label_errors_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_joint_label_errors_last_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_pack_heldout_loss.argtypes = [
        c.c_void_p, c.c_longlong, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int] + \
        [c.POINTER(c.c_void_p)] * 5
    lib.peakseg_hip_problem_set_pack_heldout_loss.restype = c.c_longlong
    lib.peakseg_hip_problem_set_packed_heldout_loss_download.argtypes = [c.c_void_p] * 6
    lib.peakseg_hip_problem_set_packed_heldout_loss_download.restype = c.c_int
    lib.peakseg_hip_heldout_loss_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_heldout_loss_last_ms.restype = c.c_int
    lib.peakseg_hip_problem_set_create_dense_folds.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.c_int, c.c_int,
        c.POINTER(c.c_double), c.c_ulonglong, c.c_int, c.c_ulonglong, c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_create_dense_folds.restype = c.c_int
    lib.peakseg_hip_problem_set_create_reads_folds.argtypes = reads + [
        c.c_int, c.POINTER(c.c_double), c.c_ulonglong, c.c_int, c.c_ulonglong, c.POINTER(c.c_void_p)]
    lib.peakseg_hip_problem_set_create_reads_folds.restype = c.c_int
    lib.peakseg_hip_fold_max_count.argtypes = []
    lib.peakseg_hip_fold_max_count.restype = c.c_int
    lib.peakseg_hip_fold_units_last_ms.argtypes = [c.POINTER(c.c_float)]
    lib.peakseg_hip_fold_units_last_ms.restype = c.c_int
    lib.peakseg_hip_reads_strand_xcorr.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.POINTER(c.c_void_p), c.c_int, c.POINTER(c.c_int),
        c.POINTER(c.c_int), c.c_int, c.c_void_p]
    lib.peakseg_hip_reads_strand_xcorr.restype = c.c_int
    lib.peakseg_hip_reads_extend.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p)]
    lib.peakseg_hip_reads_extend.restype = c.c_int
    lib.peakseg_hip_xcorr_max_shift.argtypes = []
    lib.peakseg_hip_xcorr_max_shift.restype = c.c_int
    lib.peakseg_hip_reads_last_xcorr_ms.argtypes = [c.POINTER(c.c_float), c.POINTER(c.c_float)]
    lib.peakseg_hip_reads_last_xcorr_ms.restype = c.c_int
    lib.peakseg_hip_reads_dedup.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.POINTER(c.c_void_p), c.c_int, c.c_int, c.c_int,
        c.POINTER(c.c_void_p), c.c_void_p]
    lib.peakseg_hip_reads_dedup.restype = c.c_int
    lib.peakseg_hip_reads_compact.argtypes = [
        c.c_int, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.POINTER(c.c_void_p), c.c_int] + [c.POINTER(c.c_void_p)] * 5 + [c.c_void_p]
    lib.peakseg_hip_reads_compact.restype = c.c_int
    lib.peakseg_hip_dedup_block_rows.argtypes = []
    lib.peakseg_hip_dedup_block_rows.restype = c.c_int
    lib.peakseg_hip_dedup_scan_span.argtypes = []
    lib.peakseg_hip_dedup_scan_span.restype = c.c_int
    lib.peakseg_hip_reads_last_dedup_ms.argtypes = [c.POINTER(c.c_float)] * 3
    lib.peakseg_hip_reads_last_dedup_ms.restype = c.c_int
    lib.peakseg_hip_reads_last_dedup_passes.argtypes = []
    lib.peakseg_hip_reads_last_dedup_passes.restype = c.c_int
    lib.peakseg_hip_search_place_penalties.argtypes = [
        c.c_double, c.c_double, c.c_double, c.c_int, c.POINTER(c.c_double)]
    lib.peakseg_hip_search_place_penalties.restype = c.c_int
    return lib


EXPORTED_SYMBOLS = [
    "PeakSegFPOP_disk", "PeakSegFPOP_disk_batch", "PeakSegFPOP_status_message",
    "peakseg_hip_set_print", "peakseg_hip_device_count", "peakseg_hip_last_error",
    "peakseg_hip_problem_set_create", "peakseg_hip_problem_set_solve",
    "peakseg_hip_problem_set_result", "peakseg_hip_problem_set_segments",
    "peakseg_hip_problem_set_export_db", "peakseg_hip_problem_set_bytes",
    "peakseg_hip_problem_set_destroy", "peakseg_hip_math_probe", "peakseg_hip_parse_probe",
    "peakseg_hip_math_forms_probe",
    "peakseg_hip_problem_set_profile", "peakseg_hip_problem_set_kernel_build",
    "PeakSegFPOP_dir_batch", "PeakSegFPOP_sequential_search",
    "PeakSegFPOP_sequential_search_batch",
    "peakseg_hip_problem_set_set_penalty", "peakseg_hip_problem_set_arena_bytes_used",
    "peakseg_hip_paste_double", "peakseg_hip_problem_set_checkpoint_interval",
    "peakseg_hip_problem_set_solve_stats", "peakseg_hip_device_clock_khz",
    "peakseg_hip_last_warning", "peakseg_hip_problem_set_arena_stats",
    "peakseg_hip_problem_set_park_stats", "peakseg_hip_problem_set_pack_tables",
    "peakseg_hip_problem_set_packed_download", "peakseg_hip_problem_set_cycles",
    "peakseg_hip_measured_rates", "peakseg_hip_spin_limit", "peakseg_hip_problem_set_max_spin",
    "peakseg_hip_problem_set_loop_stats",
    "peakseg_hip_last_fanout", "peakseg_hip_last_fanout_entries",
    "PeakSegFPOP_parallel_search", "PeakSegFPOP_parallel_search_batch",
    "peakseg_hip_problem_set_create_dense", "peakseg_hip_problem_set_pack_segments",
    "peakseg_hip_problem_set_packed_segments_download", "peakseg_hip_problem_set_loss",
    "peakseg_hip_dense_encode_probe", "peakseg_hip_dense_tile_bases",
    "peakseg_hip_dense_last_encode_ms",
    "peakseg_hip_problem_set_pack_segment_stats",
    "peakseg_hip_problem_set_packed_segment_stats_download",
    "peakseg_hip_segment_stats_tile_runs", "peakseg_hip_segment_stats_last_ms",
    "peakseg_hip_problem_set_create_reads", "peakseg_hip_reads_pileup_probe",
    "peakseg_hip_reads_last_pileup_ms",
    "peakseg_hip_problem_set_pack_label_errors",
    "peakseg_hip_problem_set_packed_label_errors_download",
    "peakseg_hip_label_errors_last_ms", "peakseg_hip_search_place_penalties",
    "peakseg_hip_problem_set_pack_coverage_stats",
    "peakseg_hip_problem_set_packed_coverage_stats_download",
    "peakseg_hip_coverage_stats_tile_runs", "peakseg_hip_coverage_stats_max_ranks",
    "peakseg_hip_coverage_stats_last_ms", "peakseg_hip_coverage_stats_last_passes",
    "peakseg_hip_penalty_fit", "peakseg_hip_penalty_fit_last_ms",
    "peakseg_hip_penalty_fit_max_features",
    "peakseg_hip_problem_set_pack_region_stats",
    "peakseg_hip_problem_set_packed_region_stats_download",
    "peakseg_hip_region_stats_tile_runs", "peakseg_hip_region_stats_last_ms",
    "peakseg_hip_region_stats_last_fold_grid",
    "peakseg_hip_problem_set_pack_peak_clusters",
    "peakseg_hip_problem_set_packed_peak_clusters_download",
    "peakseg_hip_peak_clusters_last_ms", "peakseg_hip_peak_clusters_probe",
    "peakseg_hip_problem_set_pack_joint_peaks",
    "peakseg_hip_problem_set_packed_joint_peaks_download", "peakseg_hip_joint_peaks_last_ms",
    "peakseg_hip_joint_path_max_penalties", "peakseg_hip_problem_set_pack_joint_path",
    "peakseg_hip_problem_set_packed_joint_path_download", "peakseg_hip_joint_path_last_ms",
    "peakseg_hip_problem_set_pack_joint_label_errors",
    "peakseg_hip_problem_set_packed_joint_label_errors_download",
    "peakseg_hip_joint_label_errors_last_ms",
    "peakseg_hip_problem_set_pack_heldout_loss",
    "peakseg_hip_problem_set_packed_heldout_loss_download", "peakseg_hip_heldout_loss_last_ms",
    "peakseg_hip_problem_set_create_dense_folds", "peakseg_hip_problem_set_create_reads_folds",
    "peakseg_hip_fold_max_count", "peakseg_hip_fold_units_last_ms",
    "peakseg_hip_reads_strand_xcorr", "peakseg_hip_reads_extend", "peakseg_hip_xcorr_max_shift",
    "peakseg_hip_reads_last_xcorr_ms",
    "peakseg_hip_reads_dedup", "peakseg_hip_reads_compact", "peakseg_hip_dedup_block_rows",
    "peakseg_hip_dedup_scan_span", "peakseg_hip_reads_last_dedup_ms",
    "peakseg_hip_reads_last_dedup_passes",
]

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "%s is missing: build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()'). "
        "peaksegdisk_amd has no CPU fallback." % LIB_PATH)

lib = declare(ctypes.CDLL(LIB_PATH))


def last_error():
    return lib.peakseg_hip_last_error().decode(errors="replace")


def last_fanout():
    """What PEAKSEG_HIP_DEVICES did in this thread's last file-level call of the library:
    {"device", "programs", "seconds"}: one item per shard (empty lists when the call did not fan
    out); "shard_of": the shard of each entry of the call, in input order (-1: none)."""
    import ctypes
    n = lib.peakseg_hip_last_fanout(0, None, None, None)
    device = (ctypes.c_int * max(n, 1))()
    programs = (ctypes.c_int * max(n, 1))()
    seconds = (ctypes.c_double * max(n, 1))()
    n = lib.peakseg_hip_last_fanout(n, device, programs, seconds)
    m = lib.peakseg_hip_last_fanout_entries(0, None)
    shard_of = (ctypes.c_int * max(m, 1))()
    lib.peakseg_hip_last_fanout_entries(m, shard_of)
    return {"device": list(device[:n]), "programs": list(programs[:n]),
            "seconds": list(seconds[:n]), "shard_of": list(shard_of[:m])}


def status_message(status, bedgraph, penalty, db):
    buf = ctypes.create_string_buffer(4096)
    lib.PeakSegFPOP_status_message(
        status, os.fsencode(bedgraph), penalty.encode(), os.fsencode(db), buf, len(buf))
    return buf.value.decode(errors="replace")
