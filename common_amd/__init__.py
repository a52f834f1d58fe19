"""common_amd -- MI355X (gfx950) implementation of the component-model scoring hot
path of datamicroscopes/common (score_value / score_data / add_value /
remove_value per row x group x feature), behind the reference's model/hypers/group
surface.  See DESIGN.md; the C ABI is include/microscopes_hip.h.

Importing the package does not touch the GPU; creating a Context does, and fails
loudly when the HIP library or a gfx950 device is missing (there is no CPU path).
"""
from ._lib import (ACC_NO_COMMIT, ACC_RESET, ACC_SUBTRACT, BB, BBNC, BNB, DD, DM, GP, NICH, NIW, NOOP,
                   HP_CLUSTER, LINKAGE_MAX_N, PRED_MASKED_ONLY, SCORE_CRP_PRIOR, MicroscopesHipError, EXPORTS, LIB_PATH, load)
from .runtime import Context, DataView, HpGrid, RelationView, SparseRelationView, State, ZMatrix, pack_hp, runtime_types_of, ss_dtype, type_of_numpy
from .chains import ChainEnsemble, JointTracker
from . import chains, diagnostics, dist, hypers, models, query, smc, tempering
from .tempering import AISResult, TemperedResult
from .smc import SMCResult
from .query import (CredibleBall, ExpectedLoss, PartitionDistances, PointEstimate, RefinedPartitions, RefinedVI, adjusted_rand, credible_ball,
                    expected_loss, partition_distances, point_estimate, refine_partition, refine_partition_vi, vi_estimate,
                    vi_table)

__all__ = ["ChainEnsemble", "JointTracker", "chains", "diagnostics", "smc", "SMCResult", "tempering", "TemperedResult", "AISResult", "Context", "DataView", "HpGrid", "hypers", "RelationView", "SparseRelationView", "State", "ZMatrix", "query", "PointEstimate", "point_estimate", "RefinedPartitions", "refine_partition", "RefinedVI", "refine_partition_vi", "vi_table", "PartitionDistances", "partition_distances", "adjusted_rand", "ExpectedLoss", "expected_loss",
           "vi_estimate", "CredibleBall", "credible_ball", "BNB", "DM", "models", "dist", "load", "MicroscopesHipError", "BB", "BBNC", "GP", "DD",
           "NICH", "NIW", "NOOP", "pack_hp", "ss_dtype", "runtime_types_of", "type_of_numpy",
           "EXPORTS", "LIB_PATH", "HP_CLUSTER", "LINKAGE_MAX_N", "PRED_MASKED_ONLY", "SCORE_CRP_PRIOR", "ACC_RESET", "ACC_SUBTRACT", "ACC_NO_COMMIT"]
