"""Drop-in for the model half of the reference's ``INR_ERD.py`` / ``prepare_qual_images.py``: ``from INR_ERD import Siren``
resolves to the soft-ERD INR on the MI355X kernels (``mri_super_resolution_amd.erd_inr.ErdSiren``), beside the helpers those
scripts define at module level.  The driver loop itself is ``mri_super_resolution_amd/scripts/INR_ERD.py``."""
import _bootstrap  # noqa: F401
from mri_super_resolution_amd.erd_inr import ErdSiren as Siren  # noqa: F401,E402
from mri_super_resolution_amd.erd_inr import (ErdFitter, calc_adc, calculate_CNR_SNR, eps, mag, noise_level,  # noqa: F401,E402
                                              soft_erd)
