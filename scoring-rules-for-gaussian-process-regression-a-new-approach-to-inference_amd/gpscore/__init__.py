"""gpscore — MI355X (gfx950) GP-regression hot path: Gram build, Cholesky /
log-determinant / solves, LOO and test-set CRPS / log-score, for the full GP and
the FITC sparse GP (Woodbury form, rows sharded over GPUs with RCCL).

Drop-in layers:
  * ``gpscore.compat``  — the reference scripts' helper functions, same names;
  * ``gpscore.GP``      — fit / predict / score on numpy arrays;
  * ``gpscore.batch``   — many small full GPs (n <= 128), or small FITC GPs (n <= 128, m <= 32,
                          the inducing inputs trained too), valued, trained and scored in one launch;
                          ``fitc_*_tall`` takes FITC problems of up to n = 2048 (kin40k's n = 500),
                          ``train_tall`` / ``value_and_grad_tall`` full GPs of up to n = 512,
                          ``blockloo_train_tall`` / ``blockloo_value_and_grad_tall`` the same on
                          the block-LOO DSS / KC objectives, ``es_train_tall`` /
                          ``es_value_and_grad_tall`` on the block-LOO energy score,
                          ``train_tall_validated`` / ``blockloo_train_tall_validated`` the tall
                          full-GP fits with a validation set scored step by step,
                          ``fitc_blockloo_*_tall`` the tall FITC problems on DSS / KC,
                          ``fitc_train_tall_validated`` / ``fitc_blockloo_train_tall_validated``
                          the tall FITC fits with a validation set scored step by step;
  * ``gpscore.dist``    — one process per GPU, FITC row sharding;
  * ``gpscore._lib``    — the ctypes binding of libgpscore.so (include/gpscore.h).
"""
from ._lib import (Context, GpsError, NotPositiveDefinite, build_id, check_build_id,  # noqa: F401
                   default_context, load, OBJ_NAMES, SCORE_NAMES)
from .gp import GP, FitResult, fit, pack_theta, score, surface  # noqa: F401
from .batch import (BatchTrainResult, FitcBatchTrainResult, blockloo_train_tall,  # noqa: F401
                    blockloo_value_and_grad_tall, es_train_tall, es_value_and_grad_tall,
                    fitc_blockloo_train_tall,
                    fitc_blockloo_value_and_grad_tall, fitc_train_batch,
                    fitc_train_tall, fitc_value_and_grad_batch, fitc_value_and_grad_tall,
                    train_batch, train_tall, value_and_grad_batch, value_and_grad_tall,
                    ValidatedTrainResult, blockloo_train_tall_validated, train_tall_validated,
                    FitcValidatedTrainResult, fitc_blockloo_train_tall_validated,
                    fitc_train_tall_validated)

__version__ = "0.1.0"
