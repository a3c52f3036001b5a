"""Model API of the reference (src/models/__init__.py:1-36): `from src.models import
FaceEnhanceNet, FaceEnhanceNetConfig, create_face_enhance_net, FaceEnhanceNetLite, RCAB,
ChannelAttention, ResidualGroup, UpsampleModule`, the discriminator (`VGGStyleDiscriminator`,
`GANLoss`, `create_discriminator`) and the ESRGAN comparison baseline (`RRDBNet`, `RRDB`,
`ResidualDenseBlock`, `ESRGANBaseline`, `create_esrgan_baseline`; inference only, esrgan.py).
The transfer model is outside this build's scope."""
from .blocks import (RCAB, ChannelAttention, PixelShuffleUpsample, ResidualGroup, UpsampleModule, icnr_init,
                     initialize_weights)
from .custom import FaceEnhanceNet, FaceEnhanceNetConfig, FaceEnhanceNetLite, create_face_enhance_net
from .discriminator import GANLoss, VGGStyleDiscriminator, create_discriminator
from .esrgan import RRDB, ESRGANBaseline, ResidualDenseBlock, RRDBNet, create_esrgan_baseline

__all__ = [
    "VGGStyleDiscriminator", "GANLoss", "create_discriminator",
    "FaceEnhanceNet", "FaceEnhanceNetLite", "FaceEnhanceNetConfig", "create_face_enhance_net",
    "RCAB", "ChannelAttention", "UpsampleModule", "ResidualGroup", "PixelShuffleUpsample",
    "icnr_init", "initialize_weights",
    "RRDBNet", "RRDB", "ResidualDenseBlock", "ESRGANBaseline", "create_esrgan_baseline",
]
