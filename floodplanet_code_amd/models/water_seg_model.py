"""WaterSegmentationModel -- MI355X drop-in for st_water_seg/models/water_seg_model.py:14-240.

Same constructor, same Lightning hook set, same state_dict keys (``model.<unet key>``), same logged metric
names; the network, the loss, the backward pass and the metric counters run in libfloodunet's HIP kernels
(floodplanet_code_amd.unet.HipUNet).  Differences, all deliberate:
  * ``training_step`` uses the fused forward+CrossEntropy kernel path; the returned loss is a torch scalar
    whose ``backward()`` (issued by Lightning's automatic optimisation, fit.py:95-97) runs the HIP backward.
  * metrics come from the confusion counts the loss kernel emits (floodplanet_code_amd.metrics), not from
    torchmetrics (absent; parity unpinned).
  * ``ignore_index=None`` is accepted and means "ignore nothing" (-100), where the reference's
    nn.CrossEntropyLoss(ignore_index=None) fails at call time.
Extra keyword arguments (not in the reference): ``precision`` ('fp32' | 'bf16' | 'fp16'), ``base_channels``,
``class_weights`` (n_classes finite values >= 0) and ``label_smoothing`` in [0, 1): the weighted, label-smoothed cross
entropy of nn.CrossEntropyLoss(weight, ignore_index, label_smoothing), in the fused loss kernels; ``focal_gamma`` >= 0:
every pixel's cross-entropy term times (1 - p[target])^focal_gamma (the focal loss; not together with label smoothing;
``loss_func`` stays the plain nn.CrossEntropyLoss); ``region_weight`` >= 0 with ``region_alpha``, ``region_beta``,
``region_smooth``: the cross entropy plus region_weight times the soft Tversky region term over all classes but the ignored
one (alpha = beta = 0.5: soft Dice, 1 and 1: soft Jaccard; fu_loss_ce_region, HipUNet.loss); ``ema_decay`` in [0, 1)
and ``ema_warmup``: an exponential moving average of the weights, updated inside the fused Adam launch, that validation and
test steps evaluate and that checkpoints carry as the top-level entry ``ema_state_dict`` (state_dict() stays the raw
weights under the reference's keys); ``grad_clip_norm`` > 0: the global L2 norm of the gradients is clipped to it inside
every optimiser step (clip_grad_norm_ ahead of Adam, on the device: HipUNet.set_grad_clip); ``weight_decay`` > 0:
torch.optim.AdamW's decoupled weight decay inside the fused Adam launch (HipUNet.set_weight_decay), on every tensor with
ndim >= 2 -- conv and head weights, not biases or BatchNorm -- or with ``decay_all`` on every tensor.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from ..lightning_compat import LightningModule
from ..metrics import SegmentationMetrics
from ..loss_options import LossOptions
from ..optim_options import OptimOptions, option_properties
from ..unet import HipAdam, HipUNet, check_class_weight, check_label_smoothing

# FU_TORCH_ADAM=1 keeps torch's own optimiser, which has none of these: the refusal of each option that is set
_TORCH_ADAM_REFUSALS = {
    "ema_decay": "the weight EMA is part of the fused Adam kernel (HipAdam): FU_TORCH_ADAM=1 together with ema_decay is not "
                 "supported",
    "grad_clip_norm": "gradient clipping runs ahead of the fused Adam kernel (HipAdam): FU_TORCH_ADAM=1 together with "
                      "grad_clip_norm is not supported",
    "weight_decay": "weight decay is part of the fused Adam kernel (HipAdam): FU_TORCH_ADAM=1 together with weight_decay is "
                    "not supported",
}


@option_properties          # ema_decay, ema_warmup, grad_clip_norm, weight_decay, decay_all: read from optim_options
class WaterSegmentationModel(LightningModule):

    def __init__(self, in_channels, n_classes, lr, log_image_iter=50, to_rgb_fcn=None, ignore_index=None,
                 optimizer_name='adam', precision='fp32', base_channels=64, class_weights=None, label_smoothing=0.0,
                 ema_decay=None, ema_warmup=True, focal_gamma=0.0, region_weight=0.0, region_alpha=0.5, region_beta=0.5,
                 region_smooth=1.0, grad_clip_norm=None, weight_decay=0.0, decay_all=False):
        super().__init__()
        # checked on the host, once; the net is armed from this one object (EMA below, clip and decay with the optimiser)
        self.optim_options = OptimOptions.make(ema_decay=ema_decay, ema_warmup=ema_warmup, grad_clip_norm=grad_clip_norm,
                                               weight_decay=weight_decay, decay_all=decay_all)
        self.n_classes = n_classes
        self.ignore_index = ignore_index
        if self.ignore_index == -1:                      # water_seg_model.py:35-36
            self.ignore_index = self.n_classes - 1
        self._loss_ignore = -100 if self.ignore_index is None else int(self.ignore_index)
        self._set_loss_options(class_weight=class_weights, label_smoothing=label_smoothing, focal_gamma=focal_gamma,
                               region_weight=region_weight, region_alpha=region_alpha, region_beta=region_beta,
                               region_smooth=region_smooth)
        self.lr = lr
        self.in_channels = in_channels
        self.optimizer_name = optimizer_name
        self.precision = precision
        self.base_channels = base_channels

        self._build_model()
        self.model.apply_optim_options(self.optim_options, step=False)   # the EMA; host bookkeeping only: the buffers are
                                                                         # made on the module's device

        self.tracked_metrics = self._get_tracked_metrics()
        self._modules["loss_func"] = self._modules.pop("loss_func")     # made first, with the checks; listed last, as ever

        self.to_rgb_fcn = to_rgb_fcn
        self.log_image_iter = log_image_iter

    def _set_loss_options(self, class_weight=None, label_smoothing=0.0, **options):
        """The one place the model's loss options are set: checked on the host before anything touches the GPU, the class
        weights kept as a tuple of plain Python numbers (checkpoint hyper_parameters), loss_func remade to match."""
        if class_weight is not None:
            class_weight = tuple(float(v) for v in check_class_weight(class_weight, self.n_classes))
        self.loss_options = LossOptions.make(self.n_classes, class_weight=class_weight,
                                             label_smoothing=check_label_smoothing(label_smoothing), **options)
        self.loss_func = nn.CrossEntropyLoss(                                  # kept for API parity (:40)
            weight=None if class_weight is None else torch.tensor(class_weight, dtype=torch.float32),
            ignore_index=self._loss_ignore, label_smoothing=self.loss_options.label_smoothing)
        return self

    def set_loss_options(self, class_weights=None, label_smoothing=0.0, focal_gamma=0.0, region_weight=0.0,
                         region_alpha=0.5, region_beta=0.5, region_smooth=1.0):
        """Replace the loss's class weights / label smoothing / focal exponent / region term after construction.  Same
        checks as the constructor."""
        return self._set_loss_options(class_weights, label_smoothing, focal_gamma=focal_gamma, region_weight=region_weight,
                                      region_alpha=region_alpha, region_beta=region_beta, region_smooth=region_smooth)

    def replace_loss_options(self, **changes):
        """set_loss_options with every option kept but those named, by LossOptions' field names (weights that are counted
        from data the model's own device context serves, fit's `--class_weights balanced`)."""
        return self._set_loss_options(**{**self.loss_options.as_kwargs(), **changes})

    class_weights = property(lambda self: self.loss_options.class_weight)
    label_smoothing = property(lambda self: self.loss_options.label_smoothing)
    focal_gamma = property(lambda self: self.loss_options.focal_gamma)
    region_weight = property(lambda self: self.loss_options.region_weight)
    region_alpha = property(lambda self: self.loss_options.region_alpha)
    region_beta = property(lambda self: self.loss_options.region_beta)
    region_smooth = property(lambda self: self.loss_options.region_smooth)

    # ------------------------------------------------------------------ construction
    def _get_tracked_metrics(self, average_mode='micro'):
        metrics = SegmentationMetrics(self.n_classes, self.ignore_index)
        self.train_metrics = metrics.clone(prefix='train_')
        self.valid_metrics = metrics.clone(prefix='val_')
        self.test_metrics = metrics.clone(prefix='test_')
        # the reference returns None here (:46-63), leaving tracked_metrics = None

    def _n_input_channels(self):
        if type(self.in_channels) is dict:
            return sum(self.in_channels.values())
        # water_seg_model.py:81-85 leaves n_in_channels unbound for a non-dict argument
        raise UnboundLocalError("local variable 'n_in_channels' referenced before assignment")

    def _build_model(self):
        self.model = HipUNet(self._n_input_channels(), self.n_classes, bilinear=True,
                             base_channels=self.base_channels, precision=self.precision)

    # ------------------------------------------------------------------ forward
    def _gather_input(self, batch):
        return batch['image']                            # water_seg_model.py:88

    def _gather_sources(self, batch):
        """What the network is fed: a tensor, or a list of tensors it sees side by side along C (EarlyFusionModel)."""
        return self._gather_input(batch)

    def forward(self, batch):
        return self.model(self._gather_sources(batch))

    def _set_model_to_train(self):
        self.model.train()

    def _set_model_to_eval(self):
        self.model.eval()

    def eval_weights(self):
        """What validation and test steps evaluate: the averaged weights when the model keeps an EMA, else the live ones.
        A context manager.  Each entry and exit re-binds the network's buffers and repacks its weights once, so a loop over
        many batches enters it once around the loop (fit_model does); a step outside such a block enters it for itself."""
        if self.ema_decay is None or self.model.ema_serving:
            return contextlib.nullcontext()
        return self.model.ema_weights()

    # the EMA travels beside state_dict(), as its own top-level checkpoint entry (Lightning calls these hooks with the
    # checkpoint dict; fit_model and the LightningModule stand-in's load_from_checkpoint do the same)
    # "ema_state_dict" has the keys of this module's state_dict() (so it loads wherever "state_dict" loads): the network's
    # entries come from the average, anything else (a loss weight buffer) is the live value.
    @staticmethod
    def _net_key(key):
        return key[6:] if key.startswith("model.") else key

    def on_save_checkpoint(self, checkpoint):
        if self.ema_decay is not None:
            ema = self.model.ema_state_dict()
            checkpoint["ema_state_dict"] = {k: ema.get(self._net_key(k), v).detach().cpu()
                                            for k, v in self.state_dict().items()}

    def on_load_checkpoint(self, checkpoint):
        ema = checkpoint.get("ema_state_dict") if isinstance(checkpoint, dict) else None
        if ema is not None and self.ema_decay is not None:
            self.model.load_ema_state_dict({self._net_key(k): v for k, v in ema.items()})

    def _fused_loss(self, batch, want_logits=False):
        """forward + CE(ignore_index) + NaN guard + argmax + confusion counts in the fused kernels.  The fp32 NCHW logits
        are only written when someone needs them: training_step's image logging is disabled in the reference
        (`if False:`, water_seg_model.py:116), so the training path never does; the counts stay on the device."""
        images = self._gather_sources(batch)
        out = self.model.loss(images, batch['target'], self._loss_ignore, return_logits=want_logits,
                              **self.loss_options.as_kwargs())
        loss, output = out if want_logits else (out, None)
        counts = self.model.pop_confusion()
        return loss, output, counts

    # ------------------------------------------------------------------ Lightning hooks
    def training_step(self, batch, batch_idx):
        self._set_model_to_train()
        loss, output, counts = self._fused_loss(batch)   # CE + NaN guard (:103-106) live in the kernel
        metric_output = self.train_metrics.update_from_counts(counts)
        self.log_dict(metric_output, prog_bar=True, on_step=True, on_epoch=True)
        return loss

    def validation_step(self, batch, batch_idx):
        self._set_model_to_eval()
        with torch.no_grad(), self.eval_weights():
            loss, output, counts = self._fused_loss(batch)
        metric_output = self.valid_metrics.update_from_counts(counts)
        self.valid_metrics.update_from_counts(counts)    # the reference counts each batch twice (:150-151)
        metric_output['valid_loss'] = loss
        self.log_dict(metric_output, prog_bar=True, on_step=True, on_epoch=True)

    def test_step(self, batch, batch_idx):
        self._set_model_to_eval()
        with torch.no_grad(), self.eval_weights():
            loss, output, counts = self._fused_loss(batch)
        self.test_metrics.update_from_counts(counts)
        self.log_dict({'test_loss': loss}, prog_bar=True, on_step=True, on_epoch=True)

    def configure_optimizers(self):
        if self.optimizer_name == 'adam':
            # optim.Adam(self.parameters(), lr=self.lr) (water_seg_model.py:200) as ONE fused kernel launch on the
            # network's flat buffers; same hyper-parameters, param_groups and state_dict layout (unet.HipAdam).
            # FU_TORCH_ADAM=1 keeps torch's own optimiser (it works on the same parameters).
            import os
            if os.environ.get("FU_TORCH_ADAM") == "1":
                for name in self.optim_options.set_fields:
                    raise NotImplementedError(_TORCH_ADAM_REFUSALS[name])
                optimizer = optim.Adam(self.parameters(), lr=self.lr)
            else:
                optimizer = HipAdam(self.model, lr=self.lr, options=self.optim_options)
        else:
            raise NotImplementedError(f'No implementation for optimizer of name: {self.optimizer_name}')
        return optimizer

    def validation_epoch_end(self, validation_step_outputs):
        if len(validation_step_outputs) == 0:
            self.test_f1_score = 0
            self.test_iou = 0
            self.test_acc = 0
        else:
            metric_output = self.valid_metrics.compute()
            self.log_dict(metric_output)

    def test_epoch_end(self, test_step_outputs) -> None:
        if len(test_step_outputs) == 0:
            return
        metric_output = self.test_metrics.compute()
        self.log_dict(metric_output)
        self.f1_score = metric_output['test_MulticlassF1Score'].item()
        self.acc = metric_output['test_MulticlassAccuracy'].item()
        self.iou = metric_output['test_MulticlassJaccardIndex'].item()

    def log_image_to_tensorflow(self, str_title, rgb_image, cm_image):
        """rgb_image, cm_image: np.array [height, width, 3]; stacked vertically and logged CHW (:227-240)."""
        log_image = np.concatenate((rgb_image, cm_image), axis=0).transpose((2, 0, 1))
        self.logger.experiment.add_image(str_title, log_image, self.global_step)
