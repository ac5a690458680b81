from .generate_random_H_large_size import draw_random_h, randomH, reference_random_h  # noqa: F401
from .homography_dataset import PairSynthesizer, val_pair  # noqa: F401
from .photometric import PhotometricAugment, draw_photometric, reference_photometric  # noqa: F401
