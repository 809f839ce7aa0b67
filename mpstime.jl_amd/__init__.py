"""mpstime.jl_amd - MI355X-native sweep engine behind MPSTime.jl's fitMPS / MPSOptions /
Encodings API.  The hot path lives in libmpstime_hip.so (csrc/); everything here is the
host-side mirror of the reference's interface for that path."""
from . import _lib
from ._lib import MPSTError, SVDError, DomainError
from .engine import SweepEngine, comm_library, sweep_batch, sweep_batch_multi, classify_batch
from .options import MPSOptions, safe_options
from .encodings import (EncodedTimeSeriesSet, Encoding, encode_dataset, model_encoding, symbolic_encoding,
                        transform_data, transform_train_data, transform_test_data, legendre_encode,
                        legendre_encode_no_norm, fourier_encode, get_fourier_freqs, angle_encode, sahand_encode,
                        uniform_encode, sahand_legendre, sahand_legendre_encode, UnivariateKDE, kde, kde_pdf, legendre,
                        legendre_no_norm, fourier, series_expand, construct_kerneldensity_wavefunction, project_legendre,
                        project_fourier, projected_legendre_encode, projected_legendre_encode_no_norm, projected_fourier_encode)
from .training import (TrainedMPS, fitMPS, fit_encoded, classify, generate_startingMPS, trendy_sine, save_trained_mps,
                       load_trained_mps, mps_content_digest)
from .distributed import Shard, split_encoded
from .imputation import (ImputationProblem, init_imputation_problem, MPS_impute, impute_dataset, kNN_impute, mar,
                         invert_test_transform, get_cdfs)
from .jld2 import JLD2File, read_jld2, load_trained_mps_jld2
from .analysis import bipartite_spectrum, single_site_spectrum, see_variation
from .analysis import PairAnalysis, pair_analysis, position_operator, mutual_information, model_correlations
from .marginal import log_marginals, class_posteriors
from .conditionals import (SiteConditionals, site_conditionals, anomaly_scores, WindowConditionals,
                           window_conditionals, window_conditionals_model, window_anomaly_scores, MarginalConditionals,
                           marginal_conditionals, marginal_conditionals_model, impute_marginal, forecast)
from .overlaps import ModelOverlaps, model_overlaps, class_overlaps
from .prefix import (EarlyClassification, prefix_log_marginals, prefix_posteriors, classify_early, early_accuracy_curve,
                     causal_scores)
from .segments import (BestSegment, segment_log_marginals, segment_posteriors, classify_segment, segment_evidence,
                       most_discriminative_segment, segment_accuracy_map)
from .rolling import (RollingForecasts, Backtest, rolling_forecasts, rolling_forecasts_model, backtest, horizon_errors_from,
                      interval_coverage_from, pinball_loss_from, valid_forecast_triangle)
from .observations import (ObservationModel, ObservedConditionals, gaussian_noise, interval_observations, observed_conditionals,
                           observed_conditionals_model, denoise, noisy_log_likelihoods, noisy_class_posteriors, classify_noisy)
from .summary import get_training_summary, training_stats, sweep_summary, print_opts
from .tuning import (tune, evaluate, eval_loss, fit_batch, BatchFit, MPSRandomSearch, TuningLoss, ClassificationLoss, MisclassificationRate,
                     BalancedMisclassificationRate, ImputationLoss, make_windows, make_stratified_cvfolds, classify_many)
from . import options

__all__ = ["SweepEngine", "comm_library", "sweep_batch", "sweep_batch_multi", "MPSOptions", "safe_options", "EncodedTimeSeriesSet", "Encoding", "encode_dataset",
           "model_encoding", "symbolic_encoding", "transform_data", "TrainedMPS", "fitMPS", "fit_encoded", "classify",
           "generate_startingMPS", "trendy_sine", "Shard", "split_encoded", "MPSTError", "SVDError", "ImputationProblem",
           "init_imputation_problem", "save_trained_mps", "load_trained_mps", "mps_content_digest", "MPS_impute", "impute_dataset", "kNN_impute", "mar", "invert_test_transform", "get_cdfs",
           "JLD2File", "read_jld2", "load_trained_mps_jld2",
           "DomainError", "bipartite_spectrum", "single_site_spectrum", "see_variation",
           "PairAnalysis", "pair_analysis", "position_operator", "mutual_information", "model_correlations",
           "classify_batch", "tune", "evaluate", "eval_loss", "fit_batch", "BatchFit", "MPSRandomSearch", "TuningLoss", "ClassificationLoss",
           "MisclassificationRate", "BalancedMisclassificationRate", "ImputationLoss", "make_windows", "make_stratified_cvfolds",
           "classify_many", "log_marginals", "class_posteriors", "SiteConditionals", "site_conditionals", "anomaly_scores", "WindowConditionals", "window_conditionals",
           "window_conditionals_model", "window_anomaly_scores", "MarginalConditionals", "marginal_conditionals", "marginal_conditionals_model",
           "impute_marginal", "forecast",
           "ModelOverlaps", "model_overlaps", "class_overlaps", "EarlyClassification", "prefix_log_marginals", "prefix_posteriors",
           "classify_early", "early_accuracy_curve", "causal_scores", "BestSegment", "segment_log_marginals", "segment_posteriors", "classify_segment",
           "segment_evidence", "most_discriminative_segment", "segment_accuracy_map", "RollingForecasts", "Backtest", "rolling_forecasts",
           "rolling_forecasts_model", "backtest", "horizon_errors_from", "interval_coverage_from", "pinball_loss_from", "valid_forecast_triangle",
           "ObservationModel", "ObservedConditionals", "gaussian_noise", "interval_observations", "observed_conditionals",
           "observed_conditionals_model", "denoise", "noisy_log_likelihoods", "noisy_class_posteriors", "classify_noisy",
           "get_training_summary", "training_stats", "sweep_summary", "print_opts",
           "sahand_legendre", "sahand_legendre_encode", "UnivariateKDE", "kde", "kde_pdf",
           "legendre", "legendre_no_norm", "fourier", "series_expand", "construct_kerneldensity_wavefunction", "project_legendre", "project_fourier",
           "projected_legendre_encode", "projected_legendre_encode_no_norm", "projected_fourier_encode"]
