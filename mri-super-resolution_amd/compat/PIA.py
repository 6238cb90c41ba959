"""Drop-in for the reference's ``PIA`` module: ``from PIA import hybrid_fit`` (superresHybrid.py:14) resolves to the MI355X
fit kernel, and ``PIA`` (the physics-informed autoencoder class), ``get_batch``, ``detect_PIDS_slice`` and ``ADC_slice``
resolve to their device implementations in ``mri_super_resolution_amd.pia_net``."""
import _bootstrap  # noqa: F401
from mri_super_resolution_amd.pia import hybrid_fit, three_compartment_fit  # noqa: F401,E402
from mri_super_resolution_amd.pia_net import PIA, ADC_slice, detect_PIDS_slice, get_batch  # noqa: F401,E402
