"""Mirror of the reference's ``utils/metrics`` package (utils/metrics/__init__.py:1-7): ``cd`` (utils/metrics/CD/__init__.py),
``fscore`` (utils/metrics/CD/fscore.py) and ``emd`` (utils/metrics/EMD/emd_module.py)."""
from .chamfer import chamfer_3D, chamfer_3DDist, chamfer_3DFunction
from .emd import emdFunction, emdModule
from .fscore import fscore

cd = chamfer_3DDist
emd = emdModule

__all__ = ["cd", "fscore", "emd", "chamfer_3D", "chamfer_3DDist", "chamfer_3DFunction", "emdFunction", "emdModule"]
