"""vi_ekf_amd -- MI355X-native batched VI-EKF predict/update core (HIP, gfx950).

The numeric path lives in libviekf_hip.so (C ABI: include/viekf.h).  Importing the package
does not need a GPU; using it does, and there is no CPU fallback.
"""
from . import capi, scene  # noqa: F401
from .batch import BatchVIEKF  # noqa: F401


def pixel_flow(batch, z_prev, ids_prev, z, ids, dt):
    """the image velocity of a frame's features from the frame before, by id, on the batch's stream (viekf_pixel_flow,
    include/viekf_pixvel.h) -> zdot [B][M][2]"""
    return batch.pixel_flow(z_prev, ids_prev, z, ids, dt)


from .capi import Params, ViekfError, device_count, load_yaml  # noqa: F401
from .seq import SeqVIEKF  # noqa: E402,F401
from .klt import KLTTracker, track_frame  # noqa: E402,F401
from . import diag  # noqa: E402,F401
from .diag import consistency, innovation  # noqa: E402,F401
from . import simbatch  # noqa: E402,F401
from .simbatch import BatchSimulator, landmarks_like  # noqa: E402,F401
from . import frame  # noqa: E402,F401
from .frame import FrameIntake  # noqa: E402,F401
from . import node  # noqa: E402,F401
from .node import NodeGraph  # noqa: E402,F401
from . import map  # noqa: E402,F401
from .map import LandmarkMap  # noqa: E402,F401
from . import rec  # noqa: E402,F401
from .rec import FlightRecorder  # noqa: E402,F401
from . import cam  # noqa: E402,F401
from .cam import CameraModel  # noqa: E402,F401
