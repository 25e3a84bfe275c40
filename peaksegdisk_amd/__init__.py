"""peaksegdisk_amd -- MI355X-native drop-in for PeakSegDisk's PeakSegFPOP hot path.

The constrained functional-pruning dynamic program of tdhock/PeakSegDisk
(src/PeakSegFPOPLog.cpp + src/funPieceListLog.cpp) as hand-written HIP kernels for gfx950
behind the reference's own entry points.  See DESIGN.md and INTEGRATION.md.
"""
from . import _native  # noqa: F401  (fails loudly when the HIP library is not built)
from .api import (PeakSegError, PeakSegFPOP_dir, PeakSegFPOP_df, PeakSegFPOP_file,  # noqa: F401
                  PeakSegFPOP_vec, PeakSegFPOP_dense, PeakSegFPOP_reads, coverage_from_reads,
                  PeakSegFPOP_dir_batch, col_name_list, paste,
                  sequentialSearch_dir, sequentialSearch_dir_batch, parallelSearch_dir,
                  parallelSearch_dir_batch, writeBedGraph, targetInterval_dense,
                  targetInterval_reads, problem_features_dense, problem_features_reads,
                  predict_penalties, consensus_peaks_dense, consensus_peaks_reads,
                  ConsensusPeaks, joint_peaks_dense, joint_peaks_reads, JointPeaks,
                  joint_target_interval_dense, joint_target_interval_reads,
                  learn_joint_penalty_dense, learn_joint_penalty_reads,
                  select_penalty_dense, select_penalty_reads, strand_cross_correlation,
                  estimate_fragment_length, extend_reads, remove_duplicates)
from ._native import last_fanout  # noqa: F401
from .grid import ProblemSet, read_labels_bed, features_from_stats  # noqa: F401
from .joint_target import JointSearch, JointTargetInterval, joint_target_interval  # noqa: F401
from .heldout import HeldoutSelection  # noqa: F401
from .strand import FragmentLength  # noqa: F401
from .dedup import DuplicateRemoval  # noqa: F401
from .fit import (PenaltyModelFit, fit_penalty_model, learn_penalty_model_dense,  # noqa: F401
                  learn_penalty_model_reads)

__all__ = ["PeakSegFPOP_file", "PeakSegFPOP_dir", "PeakSegFPOP_df", "PeakSegFPOP_vec",
           "PeakSegFPOP_dense", "PeakSegFPOP_reads", "coverage_from_reads",
           "PeakSegFPOP_dir_batch", "sequentialSearch_dir", "sequentialSearch_dir_batch",
           "parallelSearch_dir", "parallelSearch_dir_batch",
           "writeBedGraph", "col_name_list", "paste",
           "ProblemSet", "last_fanout", "read_labels_bed", "targetInterval_dense",
           "targetInterval_reads", "problem_features_dense", "problem_features_reads",
           "predict_penalties", "features_from_stats",
           "fit_penalty_model", "learn_penalty_model_dense", "learn_penalty_model_reads",
           "PenaltyModelFit", "consensus_peaks_dense", "consensus_peaks_reads", "ConsensusPeaks",
           "joint_peaks_dense", "joint_peaks_reads", "JointPeaks", "joint_target_interval_dense",
           "joint_target_interval_reads", "learn_joint_penalty_dense", "learn_joint_penalty_reads",
           "JointSearch", "JointTargetInterval", "joint_target_interval", "PeakSegError",
           "select_penalty_dense", "select_penalty_reads", "HeldoutSelection",
           "strand_cross_correlation", "estimate_fragment_length", "extend_reads", "FragmentLength",
           "remove_duplicates", "DuplicateRemoval"]
