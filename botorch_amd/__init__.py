"""botorch_amd: MI355X-native batched GP posterior + Monte-Carlo acquisition.

A drop-in for BoTorch's hot path (SingleTaskGP / GPyTorchPosterior /
MCAcquisitionFunction.forward / optimize_acqf / fit_gpytorch_mll) whose
numerics run as hand-written gfx950 HIP kernels behind the C ABI in
``include/botorch_amd.h`` (``libbotorch_amd.so``, loaded by ``_lib.py``).
"""
__version__ = "0.1.0"

# names served from their submodules on first use (importing the package
# itself loads no native library)
_EXPORTS = {"FullyBayesianAcquisitionFunction": "acquisition",
            "qBayesianActiveLearningByDisagreement": "acquisition",
            "GaussianMixturePosterior": "posteriors",
            "LogExpectedImprovement": "acquisition",
            "LogProbabilityOfImprovement": "acquisition",
            "LogConstrainedExpectedImprovement": "acquisition",
            "ConstrainedExpectedImprovement": "acquisition",
            "PosteriorStandardDeviation": "acquisition",
            "ScalarizedPosteriorMean": "acquisition",
            "fit_fully_bayesian_model_nuts": "fit",
            "FantasizedGP": "models",
            "MultiTaskGP": "models", "IndexKernel": "models", "GammaPrior": "models",
            "get_matern_kernel_with_gamma_prior": "models",
            "get_gaussian_likelihood_with_gamma_prior": "models",
            "icm_mll_terms": "fit", "icm_mll_terms_torch": "fit"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module(f"{__name__}.{_EXPORTS[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
