"""Model API of the reference (src/models/__init__.py:1-36): `from src.models import
FaceEnhanceNet, FaceEnhanceNetConfig, create_face_enhance_net, FaceEnhanceNetLite, RCAB,
ChannelAttention, ResidualGroup, UpsampleModule`, the discriminator (`VGGStyleDiscriminator`,
`GANLoss`, `create_discriminator`) and the ESRGAN comparison baseline (`RRDBNet`, `RRDB`,
`ResidualDenseBlock`, `ESRGANBaseline`, `create_esrgan_baseline`; inference only, esrgan.py) and
the transfer model (`TransferSRModel`, `TransferModelConfig`, `TrainingStage`, `FaceSpecificHead`,
`create_transfer_model`, transfer.py: the RRDB backbone + a face-specific head; inference in every
stage, training in stage 1 -- head only -- by default and in stages 2 and 3 with
`train_backbone=True`, the dense blocks' HIP backward)."""
from .blocks import (RCAB, ChannelAttention, PixelShuffleUpsample, ResidualGroup, UpsampleModule, icnr_init,
                     initialize_weights)
from .custom import FaceEnhanceNet, FaceEnhanceNetConfig, FaceEnhanceNetLite, create_face_enhance_net
from .discriminator import GANLoss, VGGStyleDiscriminator, create_discriminator
from .esrgan import RRDB, ESRGANBaseline, ResidualDenseBlock, RRDBNet, create_esrgan_baseline
from .transfer import FaceSpecificHead, TrainingStage, TransferModelConfig, TransferSRModel, create_transfer_model

__all__ = [
    "VGGStyleDiscriminator", "GANLoss", "create_discriminator",
    "FaceEnhanceNet", "FaceEnhanceNetLite", "FaceEnhanceNetConfig", "create_face_enhance_net",
    "RCAB", "ChannelAttention", "UpsampleModule", "ResidualGroup", "PixelShuffleUpsample",
    "icnr_init", "initialize_weights",
    "RRDBNet", "RRDB", "ResidualDenseBlock", "ESRGANBaseline", "create_esrgan_baseline",
    "TransferSRModel", "TransferModelConfig", "TrainingStage", "FaceSpecificHead", "create_transfer_model",
]
