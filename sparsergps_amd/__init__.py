"""sparsergps_amd -- MI355X-native sparse-GP objective + gradient (drop-in for sparseRGPs' hot path).

Product path: libsgp.so (HIP, gfx950) behind the C ABI in include/sgp.h; this package is the
host-side mirror of the reference's R/Rcpp interface for that path.
"""
from ._build import build
from ._lib import NotPositiveDefinite, SGPError
from .covariance import (cov_fun_expC, cov_fun_sqrd_exp_ardC, cov_fun_sqrd_expC, dsig_dtheta_ardC,
                         dsig_dthetaC, make_cov_mat_ardC, make_cov_matC)
from .evaluation import (joint_kl, joint_nlp, mc_nlp, my_kl, my_nlp, my_rmse, predict_prob,
                         score_gp)
from .sampling import sample_gp, sample_mvn
from .batch import (SparseGPBatch, cross_validate_gp, laplace_grad_ascent_batch,
                    norm_grad_ascent_batch, norm_grad_ascent_vi_batch, optimize_gp_batch)
from .drivers import laplace_grad_ascent, norm_grad_ascent, norm_grad_ascent_vi
from .full import (dlogp_dcov_par_full, dlogq_dcov_par_full, full_eval, full_laplace_eval,
                   laplace_grad_ascent_full, newtrapGP, norm_grad_ascent_full, obj_fun_bern_full,
                   obj_fun_norm_full, obj_fun_pois_full, predict_gp_full, predict_laplace_full)
from .optimize import optimize_gp
from .predict import predict_gp, predict_laplace, predict_vi
from .predictor import Predictor, predictor_gp
from .laplace import (dlogq_dcov_par, laplace_eval, newtrap_sparseGP, obj_fun_bern,
                      obj_fun_pois)
from .knot_selection import (oat_knot_selection, oat_knot_selection_norm,
                             oat_knot_selection_norm_vi)
from .proposals import (knot_prop_ego, knot_prop_ego_norm, knot_prop_ego_norm_vi, knot_prop_error,
                        knot_prop_random, knot_prop_random_norm, knot_prop_random_norm_vi,
                        knot_prop_var)
from .vi import (SparseGPContext, delbo_dcov_par, dlogp_dcov_par, elbo_fun, fitc_eval, param_names,
                 vi_eval)

__all__ = [
    "build", "SGPError", "NotPositiveDefinite",
    "make_cov_matC", "make_cov_mat_ardC", "dsig_dthetaC", "dsig_dtheta_ardC",
    "cov_fun_sqrd_expC", "cov_fun_sqrd_exp_ardC", "cov_fun_expC",
    "SparseGPContext", "vi_eval", "elbo_fun", "delbo_dcov_par", "param_names",
    "fitc_eval", "dlogp_dcov_par",
    "laplace_eval", "newtrap_sparseGP", "dlogq_dcov_par", "obj_fun_pois", "obj_fun_bern",
    "predict_vi", "predict_laplace", "predict_gp", "Predictor", "predictor_gp",
    "norm_grad_ascent_vi", "norm_grad_ascent", "laplace_grad_ascent",
    "full_eval", "obj_fun_norm_full", "dlogp_dcov_par_full", "norm_grad_ascent_full",
    "predict_gp_full",
    "full_laplace_eval", "newtrapGP", "obj_fun_pois_full", "obj_fun_bern_full",
    "dlogq_dcov_par_full", "laplace_grad_ascent_full", "predict_laplace_full",
    "knot_prop_ego_norm_vi", "knot_prop_ego_norm", "knot_prop_ego",
    "knot_prop_random_norm_vi", "knot_prop_random_norm", "knot_prop_random",
    "knot_prop_var", "knot_prop_error",
    "oat_knot_selection_norm_vi", "oat_knot_selection_norm", "oat_knot_selection",
    "optimize_gp",
    "SparseGPBatch", "laplace_grad_ascent_batch", "norm_grad_ascent_batch",
    "norm_grad_ascent_vi_batch", "optimize_gp_batch",
    "cross_validate_gp",
    "my_rmse", "my_nlp", "my_kl", "predict_prob", "score_gp",
    "joint_nlp", "joint_kl", "mc_nlp", "sample_mvn", "sample_gp",
]
