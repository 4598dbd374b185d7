"""A stand-in for an SD3-class (MMDiT) pipeline, for the tests of ``daam_amd.trace_joint``: a few-block transformer whose attention
modules carry exactly the attributes of diffusers' joint attention (``heads``, ``scale``, ``to_q`` / ``to_k`` / ``to_v``,
``add_q_proj`` / ``add_k_proj`` / ``add_v_proj``, ``norm_q`` / ``norm_k`` / ``norm_added_q`` / ``norm_added_k`` -- a per-head RMS norm or
``None`` --, ``to_out``, ``to_add_out``, ``processor``, ``set_processor``) with a default joint processor written with
``scaled_dot_product_attention``, and a pipeline object around it that runs classifier-free guidance as ``[uncond; cond]``.
Test-only: nothing of the product imports it.

The default processor can record what it projected (``attn.record`` a list): the kept (conditional) half of every call as f32 numpy
``(q [b, heads, P, d], k_txt [b, heads, T, d], k_img [b, heads, P, d], scale)`` -- what a float64 reference of the tap is fed."""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import fake_diffusers as fd

PATCH, VAE_SCALE, SAMPLE = 2, 8, 16                   # 16-pixel cells; the default generation is 128 x 128 pixels: an 8 x 8 grid
CLIP_ROWS, T5_ROWS = 77, 19                           # a context of 96 rows: CLIP rows first


class HeadRMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        y = x.float()
        y = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + self.eps)
        return (y * self.weight.float()).to(x.dtype)


class JointProcessor:
    """The SD3 protocol of diffusers' ``JointAttnProcessor2_0``: one softmax over image and text keys for image and text queries."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, **kw):
        batch, heads = hidden_states.shape[0], attn.heads

        def split(t, norm):
            t = t.view(batch, -1, heads, t.shape[-1] // heads)                # the norm acts on the head dim, before or after the transpose
            return (t if norm is None else norm(t)).transpose(1, 2)
        q = split(attn.to_q(hidden_states), attn.norm_q)
        k = split(attn.to_k(hidden_states), attn.norm_k)
        v = split(attn.to_v(hidden_states), None)
        cells = q.shape[2]
        if encoder_hidden_states is not None:
            cq = split(attn.add_q_proj(encoder_hidden_states), attn.norm_added_q)
            ck = split(attn.add_k_proj(encoder_hidden_states), attn.norm_added_k)
            cv = split(attn.add_v_proj(encoder_hidden_states), None)
            if attn.record is not None and attention_mask is None:
                first = batch // 2
                attn.record.append((q[first:].float().cpu().numpy(), ck[first:].float().cpu().numpy(), k[first:].float().cpu().numpy(),
                                    float(attn.scale)))
            q, k, v = torch.cat([q, cq], dim=2), torch.cat([k, ck], dim=2), torch.cat([v, cv], dim=2)
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=attention_mask, scale=attn.scale)
        out = out.transpose(1, 2).reshape(batch, -1, heads * out.shape[-1])
        if encoder_hidden_states is None:
            return attn.to_out[1](attn.to_out[0](out))
        return attn.to_out[1](attn.to_out[0](out[:, :cells])), attn.to_add_out(out[:, cells:])


class JointAttention(nn.Module):
    def __init__(self, dim, heads, qk_norm):
        super().__init__()
        d = dim // heads
        self.heads, self.scale, self.inner_dim = heads, d ** -0.5, dim
        self.to_q, self.to_k, self.to_v = (nn.Linear(dim, dim) for _ in range(3))
        self.add_q_proj, self.add_k_proj, self.add_v_proj = (nn.Linear(dim, dim) for _ in range(3))
        self.norm_q, self.norm_k, self.norm_added_q, self.norm_added_k = (HeadRMSNorm(d) if qk_norm else None for _ in range(4))
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])
        self.to_add_out = nn.Linear(dim, dim)
        self.processor = JointProcessor()
        self.record = None

    def set_processor(self, processor):
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kw):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask, **kw)


class JointBlock(nn.Module):
    def __init__(self, dim, heads, qk_norm):
        super().__init__()
        self.attn = JointAttention(dim, heads, qk_norm)


class MMDiT(nn.Module):
    """``blocks`` joint blocks with residuals; every second block has no q / k norms (SD3-medium has none, SD3.5 has them)."""

    def __init__(self, heads=2, dim_head=64, blocks=3):
        super().__init__()
        self.config = types.SimpleNamespace(sample_size=SAMPLE, patch_size=PATCH)
        self.transformer_blocks = nn.ModuleList([JointBlock(heads * dim_head, heads, qk_norm=i % 2 == 0) for i in range(blocks)])

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, hidden, context, mask=None):
        for block in self.transformer_blocks:
            dh, dc = block.attn(hidden, encoder_hidden_states=context, attention_mask=mask)
            hidden, context = hidden + dh, context + dc
        return hidden


class MMDiTPipeline:
    """``pipe(prompt, num_inference_steps, height, width)``: seeded image tokens and context per step, batch ``[uncond; cond]``.
    ``outputs`` holds what the transformer returned at every step of the last call."""

    def __init__(self, transformer, device='cpu', dtype=torch.bfloat16, seed=0, batch=2):
        self.transformer = transformer
        self.tokenizer = fd.FakeTokenizer()
        self.vae_scale_factor = VAE_SCALE
        self.device, self.dtype, self.seed, self.batch = torch.device(device), dtype, seed, batch
        self.outputs, self.checked = [], []
        self.mask_fn = None                               # optional: (tokens) -> an attention mask for every call

    def check_inputs(self, prompt, *args, **kwargs):
        self.checked.append(prompt)

    def _randn(self, *shape, key):
        g = torch.Generator(device='cpu')
        g.manual_seed((self.seed * 1000003 + key) % (2 ** 31 - 1))
        return torch.randn(*shape, generator=g).to(self.dtype).to(self.device)

    def __call__(self, prompt, num_inference_steps=2, height=None, width=None, **kw):
        size = SAMPLE * VAE_SCALE
        height, width = height or size, width or size
        self.check_inputs(prompt, None, None, height, width)
        cells = (height // (VAE_SCALE * PATCH)) * (width // (VAE_SCALE * PATCH))
        dim = self.transformer.transformer_blocks[0].attn.inner_dim
        self.outputs = []
        with torch.no_grad():
            context = self._randn(self.batch, CLIP_ROWS + T5_ROWS, dim, key=7)
            for step in range(num_inference_steps):
                hidden = self._randn(self.batch, cells, dim, key=100 + step)
                mask = None if self.mask_fn is None else self.mask_fn(cells + context.shape[1])
                self.outputs.append(self.transformer(hidden, context, mask))
        return types.SimpleNamespace(images=['image-of:' + (prompt if isinstance(prompt, str) else prompt[0])])


def make_pipe(device='cpu', dtype=torch.bfloat16, seed=0, heads=2, dim_head=64, blocks=3, batch=2):
    state = torch.get_rng_state()
    torch.manual_seed(2000 + seed)
    try:
        model = MMDiT(heads, dim_head, blocks)
    finally:
        torch.set_rng_state(state)
    return MMDiTPipeline(model.to(device=device, dtype=dtype), device, dtype, seed, batch)


def record(pipe, on=True):
    """Start (or stop) recording the projections of every joint call; returns the list they are appended to."""
    calls = [] if on else None
    for block in pipe.transformer.transformer_blocks:
        block.attn.record = calls
    return calls
