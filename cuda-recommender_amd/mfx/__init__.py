"""mfx -- Python host mirror of the MI355X-native CCD++/ALS solver (libmfx.so, include/mfx.h)."""
from . import dataset  # noqa: F401
from .api import (AlsSolver, CcdSolver, Comm, TestData, UsageError, als_gramian, als_half, als_inverse,  # noqa: F401
                  calculate_rmse_directly, device_count, extract_shard, golden_compare, initial_col,
                  kernel_wrapper_als_NV, kernel_wrapper_ccdpp_NV, parameter, parse_command_line,
                  partition_cols, partition_rows, rank_one_sweep, solvertype, test_data_of, test_rmse, update_rating)
from .api import PAD_ITEM, PAD_RANK, Recommender, ivf_kmeans, recommend, topn_metrics  # noqa: F401
from .api import ImplicitAlsSolver, ials_half, ials_block_half, ials_cg_half, spd_inverse  # noqa: F401
from .api import als_block_half  # noqa: F401
from .api import BprSolver, bpr_apply, bpr_triples  # noqa: F401
from .api import bpr_apply_neg, bpr_rank_weights, bpr_trials  # noqa: F401
from .api import LightGcnSolver, lgcn_apply, lgcn_propagate  # noqa: F401
from .api import HybFeatures, HybridSolver, hyb_apply, hyb_embed, hyb_features  # noqa: F401
from .api import ItemKnn, knn_weights  # noqa: F401
from .api import Slim, slim_gram, slim_solve  # noqa: F401
from .api import Ease, ease_gram, ease_inverse, ease_weights_from_inverse  # noqa: F401
from ._lib import LIB_PATH, MfxError, lib  # noqa: F401
from ._lib import MFX_KNN_KEEP_SEEN  # noqa: F401
from ._lib import MFX_SLIM_SIGNED  # noqa: F401
from ._lib import MFX_EASE_INV_SIMPLE  # noqa: F401
from ._lib import MFX_FOLD_ALS, MFX_FOLD_ALS_EXACT, MFX_FOLD_CCD, MFX_FOLD_IMPLICIT  # noqa: F401
from ._lib import MFX_SIM_DOT, MFX_SIM_COSINE  # noqa: F401
from ._lib import MFX_CAND_NO_EXCLUDE, MFX_DIV_NO_EXCLUDE  # noqa: F401
