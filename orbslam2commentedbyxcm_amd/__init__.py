"""orbslam2commentedbyxcm_amd -- MI355X-native ORB extraction + Hamming matching.

Drop-in for ORB-SLAM2's per-frame hot path (ORBextractor::operator(),
ORBmatcher::DescriptorDistance / SearchByProjection / SearchForTriangulation),
implemented as hand-written HIP kernels for gfx950 behind the C ABI in
include/orbx.h (liborbx.so).  This package is the host-side mirror of the
reference's ORBextractor / ORBmatcher interface.
"""
from ._lib import KEYPOINT_DTYPE, OrbxError, lib  # noqa: F401
from .covisibility import CovisibilityGraph  # noqa: F401
from .culling import MapCuller  # noqa: F401
from .loopclosing import LoopCorrector  # noqa: F401
from .database import KeyFrameDatabase  # noqa: F401
from .extractor import ORBextractor  # noqa: F401
from .initializer import Initializer  # noqa: F401
from .mapping import Triangulator  # noqa: F401
from .matcher import ORBmatcher  # noqa: F401
from .optimizer import EssentialGraphOptimizer, GlobalBundleAdjuster, LocalBundleAdjuster, PoseOptimizer, Sim3Optimizer  # noqa: F401
from .optimizer import essential_graph_edges, essential_graph_envelope  # noqa: F401
from .pnp import PnPsolver  # noqa: F401
from .sim3 import Sim3Solver  # noqa: F401
from .tracking import LocalMapTracker  # noqa: F401

__all__ = ["ORBextractor", "CovisibilityGraph", "EssentialGraphOptimizer", "GlobalBundleAdjuster", "Initializer", "KeyFrameDatabase", "LocalBundleAdjuster", "LocalMapTracker", "LoopCorrector", "MapCuller", "ORBmatcher", "PnPsolver", "PoseOptimizer", "Sim3Optimizer", "Sim3Solver", "Triangulator", "KEYPOINT_DTYPE", "OrbxError", "lib"]
