"""The tokenizer side of the reference's `models/norm_ema_quantizer.py` (NormEMAVectorQuantizer, BEiT v2 VQ-KD) on the HIP hot path.

Eval mode only -- what a frozen tokenizer runs (norm_ema_quantizer.py:149-172, 197-205): l2-normalise the features, the nearest code of
the whole codebook, the EMA of the code-usage histogram.  The indices and the histogram come from ONE launch of `xfm_vq_assign`
(csrc/vq.hip): the [M, n_embed] distance matrix of :158-160, its argmin (:162) and the one-hot matrix of :166 are never built.  z_q and
the commitment loss are a few torch lines on the indices, off the hot path (`VQKD.get_tokens` discards them).

Parameter and buffer names are the reference's (`embedding.weight`, `embedding.cluster_size`, `embedding.embed_avg`, `embedding.initted`,
`cluster_size`), so a tokenizer checkpoint loads unchanged.  Training the tokenizer (the EMA codebook update :174-194, k-means
initialisation :90-98, the distributed all-reduce of the histogram :138-140) raises NotImplementedError.
"""
import torch
import torch.distributed as distributed
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fx


class EmbeddingEMA(nn.Module):
    """norm_ema_quantizer.py:64-117, the containers and the lookup."""

    def __init__(self, num_tokens, codebook_dim, decay=0.99, eps=1e-5, kmeans_init=True, codebook_init_path=''):
        super().__init__()
        if codebook_init_path != '':
            raise NotImplementedError("codebook_init_path (norm_ema_quantizer.py:78-82): load a state_dict instead")
        self.num_tokens, self.codebook_dim, self.decay, self.eps = num_tokens, codebook_dim, decay, eps
        if not kmeans_init:
            weight = F.normalize(torch.randn(num_tokens, codebook_dim), p=2, dim=-1)
        else:
            weight = torch.zeros(num_tokens, codebook_dim)
        self.register_buffer('initted', torch.Tensor([not kmeans_init]))
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.cluster_size = nn.Parameter(torch.zeros(num_tokens), requires_grad=False)
        self.embed_avg = nn.Parameter(weight.clone(), requires_grad=False)
        self.update = True

    def forward(self, embed_id):
        return F.embedding(embed_id, self.weight)


class NormEMAVectorQuantizer(nn.Module):
    def __init__(self, n_embed, embedding_dim, beta, decay=0.99, eps=1e-5, statistic_code_usage=True, kmeans_init=False,
                 codebook_init_path=''):
        super().__init__()
        self.codebook_dim = embedding_dim
        self.num_tokens = n_embed
        self.beta = beta
        self.decay = decay
        self.embedding = EmbeddingEMA(self.num_tokens, self.codebook_dim, decay, eps, kmeans_init, codebook_init_path)
        self.statistic_code_usage = statistic_code_usage
        if statistic_code_usage:
            self.register_buffer('cluster_size', torch.zeros(n_embed))
        self._initted_seen = False   # `embedding.initted` is read from the device ONCE, on the first call after construction or a load
        self.register_load_state_dict_post_hook(lambda mod, keys: setattr(mod, "_initted_seen", False))

    def reset_cluster_size(self, device):
        if self.statistic_code_usage:
            self.register_buffer('cluster_size', torch.zeros(self.num_tokens))
            self.cluster_size = self.cluster_size.to(device)

    def _checks(self):
        if self.training:
            raise NotImplementedError("NormEMAVectorQuantizer: training the tokenizer (the EMA codebook update, norm_ema_quantizer.py:174-194) "
                                      "is out of scope; call .eval()")
        if distributed.is_available() and distributed.is_initialized() and distributed.get_world_size() > 1 and self.statistic_code_usage:
            raise NotImplementedError("NormEMAVectorQuantizer: the all-reduce of the code-usage histogram (norm_ema_quantizer.py:138-140, 171)")

    def assign(self, z_flat):
        """z_flat fp32 [M, codebook_dim] (not yet normalised) -> indices int64 [M]; the eval-mode EMA of cluster_size (:168-172)."""
        self._checks()
        counts = None
        if self.statistic_code_usage:
            counts = torch.zeros(self.num_tokens, dtype=torch.int32, device=z_flat.device)
        z_flat = z_flat.float()
        if z_flat.stride(-1) != 1 or z_flat.stride(0) % 4 or z_flat.data_ptr() % 16:
            z_flat = z_flat.contiguous()
        if not self._initted_seen:   # :156 init_embed_ would run k-means on an un-initted codebook (one host read, not one per step)
            if not bool(self.embedding.initted):
                raise NotImplementedError("NormEMAVectorQuantizer: k-means initialisation of the codebook (norm_ema_quantizer.py:90-98, 156) is "
                                          "out of scope; load a trained codebook (its `embedding.initted` is 1)")
            self._initted_seen = True
        idx = Fx.vq_assign(z_flat, self.embedding.weight, counts=counts)
        if counts is not None:
            with torch.no_grad():
                self.cluster_size.mul_(self.decay).add_(counts.to(self.cluster_size.dtype), alpha=1 - self.decay)
        return idx

    def forward(self, z):
        """z [b, c, h, w] -> (z_q [b, c, h, w], loss, encoding_indices [b*h*w]) as norm_ema_quantizer.py:149-205 in eval mode."""
        z = z.permute(0, 2, 3, 1)
        encoding_indices = self.assign(z.reshape(-1, self.codebook_dim))
        z = F.normalize(z, p=2, dim=-1)
        z_q = self.embedding(encoding_indices).view(z.shape)
        loss = self.beta * F.mse_loss(z_q.detach(), z)
        z_q = z + (z_q - z).detach()
        return z_q.permute(0, 3, 1, 2), loss, encoding_indices
