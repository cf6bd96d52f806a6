"""MI355X-native EM hot path of ngsF-HMM behind a C ABI (include/nghmm.h).

The directory name contains a hyphen, so import it with
``importlib.import_module("ngsf-hmm_amd")``.

This package holds only what the hot path needs:

* ``csrc/``       hand-written HIP kernels for gfx950, the L-BFGS-B state machines and
                  the C-ABI implementation -> ``libnghmm.so`` (built in-tree);
* ``hmm.py``      host-side mirror of the reference's EM interface (EM, iter_EM,
                  forward/backward/viterbi semantics) over ctypes;
* ``simulate.py`` synthetic inputs restating scripts/ngsF-HMMsim.R.

There is no CPU fallback: if ``libnghmm.so`` or a HIP device is missing, creating
an :class:`NgsFHMM` raises.
"""
from .hmm import (NgsFHMM, NgsFHMMError, Group, Chain, MODE_EXACT, MODE_FAST, GENO_PACKED, LD_INTENDED, EPROB_LD, library_path,
                  load_library,
                  build_library, bed_lines, TRACTS_VITERBI, TRACTS_POSTERIOR, PATH_STATS_DTYPE,
                  path_stats_summary, INFO_DTYPE, std_errors, SUMMARY_VITERBI, SUMMARY_POSTERIOR,
                  SUMMARY_SEGMENT_SITES, REGION_STAT_DTYPE, SITE_STAT_DTYPE, chromosome_regions,
                  window_regions, SHARING_VITERBI, SHARING_POSTERIOR, SHARING_SPLIT_SITES,
                  sharing_splits, sharing_jaccard, TractScore, TRACT_SCORE_DTYPE, TractBound,
                  TRACT_BOUND_DTYPE, NO_ANCHOR, FREQ_STAT_DTYPE, freq_std_errors,
                  GENO_SITE_STAT_DTYPE, GENO_REGION_STAT_DTYPE, geno_em_freq, het_outside_ibd,
                  EXPECT_VITERBI, EXPECT_REGION_DTYPE, EXPECT_SITE_DTYPE, expect_tract_length,
                  MOMENTS_MB, MOMENT_REGION_DTYPE, moment_sd,
                  BYLENGTH_MB, BYLENGTH_DTYPE, by_length_classes,
                  LONG_MB, LONG_REGION_DTYPE, LONG_SITE_DTYPE, long_tracts,
                  LONGEST_MB, LONGEST_DTYPE, longest_classes, COUNT_MB, count_summary,
                  LONG_MOMENTS_MB, LONG_MOMENT_DTYPE, long_moment_sd)
from . import simulate

__all__ = ["NgsFHMM", "NgsFHMMError", "Group", "Chain", "MODE_EXACT", "MODE_FAST", "GENO_PACKED", "LD_INTENDED", "EPROB_LD", "library_path",
           "load_library", "build_library", "simulate", "bed_lines", "TRACTS_VITERBI", "TRACTS_POSTERIOR",
           "PATH_STATS_DTYPE", "path_stats_summary", "INFO_DTYPE", "std_errors", "SUMMARY_VITERBI",
           "SUMMARY_POSTERIOR", "SUMMARY_SEGMENT_SITES", "REGION_STAT_DTYPE", "SITE_STAT_DTYPE",
           "chromosome_regions", "window_regions", "SHARING_VITERBI", "SHARING_POSTERIOR",
           "SHARING_SPLIT_SITES", "sharing_splits", "sharing_jaccard", "TractScore",
           "TRACT_SCORE_DTYPE", "TractBound", "TRACT_BOUND_DTYPE", "NO_ANCHOR",
           "FREQ_STAT_DTYPE", "freq_std_errors", "GENO_SITE_STAT_DTYPE", "GENO_REGION_STAT_DTYPE",
           "geno_em_freq", "het_outside_ibd", "EXPECT_VITERBI", "EXPECT_REGION_DTYPE",
           "EXPECT_SITE_DTYPE", "expect_tract_length", "MOMENTS_MB", "MOMENT_REGION_DTYPE",
           "moment_sd", "BYLENGTH_MB", "BYLENGTH_DTYPE", "by_length_classes",
           "LONG_MB", "LONG_REGION_DTYPE", "LONG_SITE_DTYPE", "long_tracts",
           "LONGEST_MB", "LONGEST_DTYPE", "longest_classes", "COUNT_MB", "count_summary",
           "LONG_MOMENTS_MB", "LONG_MOMENT_DTYPE", "long_moment_sd"]
