"""The virtual-adversarial power iteration, once, for every model family.

The reference writes it three times (UNet_VAT, model/UNet_onset.py:101-162; stepwise_VAT and stepwise_VAT_frame_stack,
model/onset_frame_VAT.py:158-269).  The three differ in which model outputs are compared, in the distance, in the factor the
gradient is scaled by and in the shape of what they return; the classes of those names (``model.UNet_VAT``,
``onset_frames.stepwise_VAT*``) supply exactly that and inherit everything else from ``VAT``.
"""
import torch
import torch.nn as nn

from . import ops
from .ops import VatPerturbFn


def zero_loss():
    """The term of a branch that did not run (no unlabelled batch, VAT off): a CPU zero, as in the reference --
    train.weighted_loss adds host terms on the host and device terms on the device."""
    return torch.tensor(0.)


class VAT(nn.Module):
    """n_power power iterations (forward on x + XI*d with detached weights, input-gradient backward), the adversarial input
    x + epsilon * d/||d||, and the grad-enabled pass on it.  The reference back-propagates the power-iteration loss into the
    weights and then discards those gradients with ``model.zero_grad()``; here the weights are detached for that pass, so only
    the input-gradient chain runs (identical ``d.grad``).  n_power = 0: the loop body never runs in the reference either, d stays
    the random draw and r_adv = eps * d / ||d|| is a RANDOM, not adversarial, perturbation.

    A subclass gives ``outputs`` / ``terms`` / ``package`` and may set ``scale`` and ``nan_message``."""
    scale = 1e10                   # d = d.grad * scale before the normalisation
    nan_message = 'r_adv contains nan'

    def __init__(self, XI, epsilon, n_power):
        super().__init__()
        self.n_power, self.XI, self.epsilon = n_power, XI, epsilon
        self.nan_flag = None
        self.noise = None          # optional callable(x) -> d0 (tests inject deterministic noise)

    def outputs(self, model, x, detach=False):
        """The tuple of predictions that are compared (detach: with detached weights)."""
        raise NotImplementedError

    def terms(self, preds, refs):
        """The distance terms, launched in list order."""
        raise NotImplementedError

    def package(self, terms):
        """What the final pass's terms are returned as."""
        raise NotImplementedError

    def power_iteration(self, model, x, refs=None):
        """Everything of the VAT call that needs no weight gradients: the target predictions (`refs`: ``outputs(model, x)`` if
        the caller already has them -- run_on_batch reuses its main forward pass, see model._Base._vat_reusing_forward), the
        power iteration and the adversarial input.  Returns (x_adv, r_adv, d_normalised, refs)."""
        if self.nan_flag is None or self.nan_flag.device != x.device:
            self.nan_flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        if refs is None:
            with torch.no_grad():
                refs = self.outputs(model, x)
        else:
            refs = tuple(r.detach() for r in refs)
        d = (self.noise(x) if self.noise is not None else torch.randn_like(x)).requires_grad_(True)
        g = None
        for it in range(self.n_power):
            if it > 0:
                d = (g * self.scale).requires_grad_(True)
            x_adv = VatPerturbFn.apply(x, d, float(self.XI))
            loss = None
            for term in self.terms(self.outputs(model, x_adv, detach=True), refs):
                loss = term if loss is None else loss + term
            g, = torch.autograd.grad(loss, d)
            g = g.detach()
        d, prescale = (d.detach(), 1.0) if g is None else (g, self.scale)
        x_adv, r_adv, d_norm = ops.vat_adversarial(x, d, prescale, float(self.epsilon), self.nan_flag)
        return x_adv, r_adv, d_norm, refs

    def check_nan(self):
        if not torch.cuda.is_current_stream_capturing():     # a captured step reads the flag in train.TrainStep.check
            assert int(self.nan_flag.item()) == 0, self.nan_message

    def final_loss(self, model, x_adv, refs):
        """The grad-enabled pass on the adversarial input and its distance to the target predictions."""
        return self.package(self.terms(self.outputs(model, x_adv), refs))

    def forward(self, model, x, refs=None, check=True):
        x_adv, r_adv, d_norm, refs = self.power_iteration(model, x, refs)
        if check:
            self.check_nan()
        return self.final_loss(model, x_adv, refs), r_adv, d_norm
