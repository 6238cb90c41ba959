"""Drop-in for the reference's ``INRmodel`` module (inrDWI.py:9): same symbols as ``SRDWI`` but
``Siren`` follows INRmodel.py:122-151 -- head constructed last (different RNG draw order), no
``first_omega_0`` keyword, coordinates not detached.  ``ComplexGaborLayer2D`` (INRmodel.py:66-120) is the layer of ``wire``:
inference through the kernels, training through ``wire.WireFitter``."""
import _bootstrap  # noqa: F401
from mri_super_resolution_amd import inr as _inr  # noqa: E402
from mri_super_resolution_amd.inr import (ImageFitting_set, PN, SineLayer, calculate_ADC,  # noqa: F401,E402
                                          calculate_combinations, get_mgrid, input_mapping, resize_array)
from mri_super_resolution_amd.wire import ComplexGaborLayer2D  # noqa: F401,E402


class Siren(_inr.Siren):
    def __init__(self, in_features, hidden_features, hidden_layers, out_features, hidden_omega_0=30.):
        super().__init__(in_features, hidden_features, hidden_layers, out_features, 30., hidden_omega_0,
                         flavor="INRmodel")
