from bodywork_mlops_demo_amd.models import conformal
from bodywork_mlops_demo_amd.models.conformal import Calibration  # noqa: F401
from bodywork_mlops_demo_amd.models.linear import GPULinearRegressor  # noqa: F401
from bodywork_mlops_demo_amd.models.mlp import GPUMLPRegressor  # noqa: F401
from bodywork_mlops_demo_amd.models.poly import (  # noqa: F401
    GPUPolyRegressor,
    GPUPolyRegressorCV,
)


def regressor_from_artifact(obj, device="cpu"):
    """Rehydrate any supported joblib artefact onto a device.

    Accepts the sklearn estimators this framework emits for artefact
    compatibility (LinearRegression, MLPRegressor, the
    PolynomialFeatures+Ridge Pipeline) as well as its own estimator
    classes.  A ``conformal_`` dict on the artefact comes back as the
    regressor's :class:`Calibration`.
    """
    if isinstance(obj, (GPULinearRegressor, GPUMLPRegressor,
                        GPUPolyRegressor)):
        return obj.to(device)
    cls = type(obj).__name__
    if cls == "LinearRegression":
        model = GPULinearRegressor.from_sklearn(obj, device)
    elif cls == "MLPRegressor":
        model = GPUMLPRegressor.from_sklearn(obj, device)
    elif cls == "Pipeline" and "ridge" in getattr(obj, "named_steps", {}):
        model = GPUPolyRegressor.from_sklearn(obj, device)
    else:
        raise TypeError(f"unsupported model artefact type: {type(obj)!r}")
    calibration = conformal.restore(obj)
    if calibration is not None:
        model.conformal_ = calibration
    return model
