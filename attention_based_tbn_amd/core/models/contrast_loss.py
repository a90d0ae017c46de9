"""ContrastLoss on the attention weights -- mirrors reference core/models/contrast_loss.py:4-25.
The definition of the term: TBNModel.get_loss evaluates it (with the prior and entropy terms) in the HIP operator
ops.attn_regularisers (tbn_attn_reg_fwd / _bwd) when the weights are float32 on the GPU and the reduction is mean or
batchmean; this module runs on CPU tensors, for the unreduced reduction="sum" vector and whenever the operator does not
cover the criterion table (TBNModel._fused_attention_losses returns None)."""
import torch.nn as nn


class ContrastLoss(nn.Module):
    def __init__(self, threshold=0.5, reduction=None):
        super().__init__()
        self.threshold = threshold
        if reduction not in ("mean", "batchmean", "sum"):
            raise Exception(f"{reduction} type reduction not supported for Contrast Loss")
        self.reduction = reduction

    def forward(self, input):
        hi = input.detach() >= self.threshold          # weights already above the threshold are pushed up
        signed = input.masked_fill(hi, 0) - input.masked_fill(~hi, 0)
        loss = signed.sum(dim=1)
        if self.reduction in ("mean", "batchmean"):
            loss = loss.mean()
        return loss
