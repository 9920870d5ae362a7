"""MI355X-native heterogeneous-GNN message passing: drop-in for the hot path of
AdalineL/Multi-Modal-GNN (``src/model.py`` HeteroRGCN on the ``edge_index`` contract of
``src/graph_build.py``).  Python host over hand-written HIP kernels (libmmgnn.so, C ABI in
``include/mmgnn.h``).  There is no CPU fallback: the ops raise if the library is missing.
"""
from . import _lib  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # lazy: keep `import mmgnn` cheap and free of torch for tools that only need the C ABI table
    if name in ("build_model", "HeteroRGCN", "EdgeRegressionHead", "compute_regression_loss"):
        from . import model
        return getattr(model, name)
    if name in ("HeteroGraph",):
        from . import data
        return getattr(data, name)
    if name in ("preprocess_lab_events", "aggregate_lab_values", "normalize_lab_values", "remove_outliers",
                "LabNormalizer", "select_codes", "filter_labs_for_cohort", "process_diagnoses", "process_medications",
                "normalize_drug_name", "preprocess_frames"):
        from . import preprocess
        return getattr(preprocess, name)
    if name in ("run_analysis", "create_per_lab_calibration_table", "create_error_vs_degree_table",
                "parity_by_frequency_decile"):
        from . import analysis
        return getattr(analysis, name)
    if name in ("embedding_maps", "lab_panels", "PCAResult", "embedding_tsne", "tsne", "TSNEResult"):
        from . import embed
        return getattr(embed, name)
    if name in ("LabConformal", "fit_conformal", "conformal_report", "impute_intervals"):
        from . import conformal
        return getattr(conformal, name)
    if name in ("BootstrapResult", "bootstrap_metrics", "evaluate_with_intervals", "poisson_weights"):
        from . import bootstrap
        return getattr(bootstrap, name)
    if name in ("ShiftResult", "two_sample", "split_shift", "residual_shift", "triples_shift"):
        from . import shift
        return getattr(shift, name)
    if name in ("LabPropensity", "measurement_features", "missingness_report", "ipw_metrics", "IpwMetrics"):
        from . import missingness
        return getattr(missingness, name)
    raise AttributeError(name)
