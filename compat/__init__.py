"""`import compat` (repository root on sys.path): the shim's helpers.  The directory itself is what goes on sys.path for the
reference's module names -- see README.md beside this file."""
from gfnet_amd.model.crossview_decoder import CrossViewDecoder  # noqa: F401
from gfnet_amd.model.dinov2 import DinoVisionTransformer  # noqa: F401
from gfnet_amd.model.fpn import Conv2d, FPNDecoder_concat, FPNEncoder, Swish, merge_layer  # noqa: F401
from gfnet_amd.reference_backbone import ReferenceBackbone, checkout_available, reference_backbone  # noqa: F401

from ._shim import OVERRIDES, install_finder  # noqa: F401
