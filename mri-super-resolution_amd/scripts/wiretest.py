#!/usr/bin/env python3
"""``wiretest.ipynb`` of the reference (implicit-neural-representations/wiretest.ipynb) as a driver on the MI355X path: the
WIRE complex-Gabor network (cells 1-2, 7) fitted by cell 10's whole loop, the PerturbNet tail included.

The flags are ``superresDWI``'s, the defaults the notebook's (cells 6-8): ``--mapping_size 256 --scale 0.5 --hidden_dim 256
--num_layers 3 --PN_dim 128 --roi_start 45 --roi_end 75 --number_of_epochs 2500 --pertubation_epochs 3 --learning_rate 5e-5
--wire_omega 1.2 --wire_scale 1.2``; the network is ``Wire(2 * mapping_size, hidden_dim // 2, num_layers, 1)``.  Inputs:
  * a ``master.mat`` with ``hybrid_raw`` -- the notebook's own format: acquisition products, mean image, then
    ``drivers.fit_wire_with_perturbnet`` (plain Adam steps on the mean image; in the last ``--pertubation_epochs`` epochs odd
    ones take one more INR step, even ones one PerturbNet step per acquisition product, the gradient flowing WIRE input ->
    Fourier features -> PerturbNet);
  * a plain volume [X, Y, Z] or [X, Y, Z, b]: the plain fit only (there are no single acquisitions to perturb towards).
Outputs: the files of ``superresDWI --model wire`` (``recon.mat`` / ``recon.npy``, ``ssim_scores.csv``, ``metrics.json``, the
optional ``--transverse_length`` / ``--adc`` products); ``metrics.json`` gains ``pn_steps`` (PerturbNet updates taken) and
``pn_final_loss`` (the loss of the last one; null when none was taken).  ``--wire_derivative_maps`` adds ``derivatives.mat`` as
in ``superresDWI --model wire``; ``--derivative_maps``, the SIREN's flag, stays refused, and so are ``--lr_model average`` and
``--footprint box``, which the parser inherits: the WIRE fit and the PerturbNet phase are point-sampled on the decimation grid
(``superresDWI._check_footprint``, reached through ``run_patient`` before the input is loaded).  Loading, re-sampling, evaluation and
writing are ``superresDWI``'s own functions, so ``--denoise mppca [--denoise_window a b c]`` (MP-PCA denoising of the raw stack before
the per-cell normalisation) and ``--degibbs`` (Gibbs-ringing removal after it) are inherited with them.
"""
from __future__ import annotations

import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
from mri_super_resolution_amd import drivers, wire  # noqa: E402
from mri_super_resolution_amd.scripts import superresDWI as dwi  # noqa: E402

NOTEBOOK_DEFAULTS = dict(mapping_size=256, scale=0.5, hidden_dim=256, num_layers=3, PN_dim=128, roi_start=45, roi_end=75,
                         number_of_epochs=2500, pertubation_epochs=3, learning_rate=5e-5, wire_omega=1.2, wire_scale=1.2,
                         model="wire")


def build_parser():
    p = dwi.build_parser()
    p.description = "WIRE super-resolution of diffusion MRI volumes with the PerturbNet phase (wiretest.ipynb protocol)"
    p.set_defaults(**NOTEBOOK_DEFAULTS)
    return p


def check_model(args):
    """Refuses what the WIRE path does not serve, before the input is loaded and anything touches the device.  Returns None:
    an input with single acquisitions is served (the PerturbNet phase)."""
    if args.model != "wire":
        raise ValueError("wiretest fits the WIRE network only (--model wire); the SIREN's driver is superresDWI")
    if args.pertubation_epochs < 0:
        raise ValueError(f"--pertubation_epochs must be >= 0 (got {args.pertubation_epochs})")
    dwi._check_wire(args)
    return None


def fit(args, INR, B, mean_dataset, model_input, target, acq_lr):
    """Cell 10: -> (losses, what ``metrics.json`` gains)."""
    if acq_lr is None:
        _, losses = wire.fit_wire(INR, model_input, target, args.number_of_epochs, lr=args.learning_rate)
        return losses, {"pn_steps": 0, "pn_final_loss": None}
    f = drivers.fit_wire_with_perturbnet
    losses = f(INR, B, mean_dataset, acq_lr, args.number_of_epochs, args.pertubation_epochs, PN_dim=args.PN_dim,
               lr=args.learning_rate)
    return losses, {"pn_steps": int(f.last_pn_steps), "pn_final_loss": f.last_pn_losses[-1] if f.last_pn_losses else None}


def run_patient(path, pt_id, args):
    return dwi.run_patient(path, pt_id, args, check_model=check_model, fit=fit)


def main(argv=None):
    return dwi.main(argv, parser=build_parser(), run=run_patient)


if __name__ == "__main__":
    main()
