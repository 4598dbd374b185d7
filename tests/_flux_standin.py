"""A stand-in for a FLUX-class pipeline, for the tests of ``daam_amd.trace_flux``, on the pattern of ``_mmdit_standin``: a transformer of
double-stream blocks (``transformer_blocks``: joint attention of image and text streams) and single-stream blocks
(``single_transformer_blocks``: one sequence ``[text; image]`` attends to itself) whose attention modules carry the attributes of
diffusers' FLUX attention and whose default processor follows ``FluxAttnProcessor2_0``: projections, per-head RMS norms (or ``None``),
text rows first, the rotary embedding in interleaved-pair form on Q and K, ``scaled_dot_product_attention``.  The pipeline object
builds FLUX's real cos / sin table for its grid (``_rope_domain.flux_table``).  Test-only: nothing of the product imports it.

The default processor can record (``attn.record`` a list) the post-rotary, dtype-rounded tensors its softmax saw, as f32 numpy
``(kind, q [1, heads, P, d], k_txt [1, heads, T, d], k_img [1, heads, P, d], scale)`` -- what a float64 reference of the tap is fed."""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

import _rope_domain as R
from _mmdit_standin import HeadRMSNorm
from oracle import fake_diffusers as fd

CELL = 16                                             # pixels a token covers on a side; the default generation is 128 x 128: 8 x 8 cells
SIZE = 128
T5_ROWS = 19


class FakeSentencePiece:
    """``tokenize`` in the manner of T5's sentencepiece model: a word-start marker on the first piece of every word, a word of more
    than 4 letters that ends in 's' split before the 's', a comma as a marker piece of its own followed by ','."""

    def tokenize(self, text):
        pieces = []
        for word in text.replace(',', ' ,').split():
            if word == ',':
                pieces += ['▁', ',']
            elif len(word) > 3 and word.endswith('s'):
                pieces += ['▁' + word[:-1], 's']
            else:
                pieces.append('▁' + word)
        return pieces


def apply_rotary(x, cos, sin):
    """diffusers' ``apply_rotary_emb(x, (cos, sin), use_real=True, use_real_unbind_dim=-1)`` on x [b, heads, rows, d]."""
    c, s = cos[None, None], sin[None, None]
    real, imag = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    turned = torch.stack([-imag, real], dim=-1).flatten(3)
    return (x.float() * c + turned.float() * s).to(x.dtype)


class FluxProcessor:
    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None):
        batch, heads = hidden_states.shape[0], attn.heads

        def split(t, norm):
            t = t.view(batch, -1, heads, t.shape[-1] // heads)
            return (t if norm is None else norm(t)).transpose(1, 2)
        q = split(attn.to_q(hidden_states), attn.norm_q)
        k = split(attn.to_k(hidden_states), attn.norm_k)
        v = split(attn.to_v(hidden_states), None)
        text = T5_ROWS
        if encoder_hidden_states is not None:
            text = encoder_hidden_states.shape[1]
            cq = split(attn.add_q_proj(encoder_hidden_states), attn.norm_added_q)
            ck = split(attn.add_k_proj(encoder_hidden_states), attn.norm_added_k)
            cv = split(attn.add_v_proj(encoder_hidden_states), None)
            q, k, v = torch.cat([cq, q], dim=2), torch.cat([ck, k], dim=2), torch.cat([cv, v], dim=2)      # text rows first
        if image_rotary_emb is not None:
            q, k = apply_rotary(q, *image_rotary_emb), apply_rotary(k, *image_rotary_emb)
        if attn.record is not None and attention_mask is None and batch == 1:
            attn.record.append(('single' if encoder_hidden_states is None else 'double', q[:, :, text:].float().cpu().numpy(),
                                k[:, :, :text].float().cpu().numpy(), k[:, :, text:].float().cpu().numpy(), float(attn.scale)))
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=attention_mask, scale=attn.scale)
        out = out.transpose(1, 2).reshape(batch, -1, heads * out.shape[-1])
        if encoder_hidden_states is None:
            return out                                                        # a single-stream block projects outside its attention
        return attn.to_out[1](attn.to_out[0](out[:, text:])), attn.to_add_out(out[:, :text])


class FluxAttention(nn.Module):
    def __init__(self, dim, heads, qk_norm, pre_only):
        super().__init__()
        d = dim // heads
        self.heads, self.scale, self.inner_dim = heads, d ** -0.5, dim
        self.to_q, self.to_k, self.to_v = (nn.Linear(dim, dim) for _ in range(3))
        self.norm_q, self.norm_k = (HeadRMSNorm(d) if qk_norm else None for _ in range(2))
        if not pre_only:
            self.add_q_proj, self.add_k_proj, self.add_v_proj = (nn.Linear(dim, dim) for _ in range(3))
            self.norm_added_q, self.norm_added_k = (HeadRMSNorm(d) if qk_norm else None for _ in range(2))
            self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])
            self.to_add_out = nn.Linear(dim, dim)
        self.processor = FluxProcessor()
        self.record = None

    def set_processor(self, processor):
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              image_rotary_emb=image_rotary_emb)


class DoubleBlock(nn.Module):
    def __init__(self, dim, heads, qk_norm):
        super().__init__()
        self.attn = FluxAttention(dim, heads, qk_norm, pre_only=False)


class SingleBlock(nn.Module):
    def __init__(self, dim, heads, qk_norm):
        super().__init__()
        self.attn = FluxAttention(dim, heads, qk_norm, pre_only=True)
        self.proj_out = nn.Linear(dim, dim)


class FluxTransformer(nn.Module):
    """``double`` double-stream then ``single`` single-stream blocks with residuals; the second block of each kind has no q / k norms."""

    def __init__(self, heads=2, dim_head=64, double=2, single=2):
        super().__init__()
        self.config = types.SimpleNamespace(axes_dims_rope=R.AXES[dim_head] if dim_head in R.AXES else None)
        self.transformer_blocks = nn.ModuleList([DoubleBlock(heads * dim_head, heads, qk_norm=i % 2 == 0) for i in range(double)])
        self.single_transformer_blocks = nn.ModuleList([SingleBlock(heads * dim_head, heads, qk_norm=i % 2 == 0) for i in range(single)])

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, hidden, context, rotary=None, mask=None):
        for block in self.transformer_blocks:
            dh, dc = block.attn(hidden, encoder_hidden_states=context, attention_mask=mask, image_rotary_emb=rotary)
            hidden, context = hidden + dh, context + dc
        x = torch.cat([context, hidden], dim=1)
        for block in self.single_transformer_blocks:
            x = x + block.proj_out(block.attn(x, attention_mask=mask, image_rotary_emb=rotary))
        return x[:, context.shape[1]:]


class FluxPipeline:
    """``pipe(prompt, prompt_2, num_inference_steps, height, width)``: seeded image tokens and a T5 context per step, batch 1 (FLUX
    runs no ``[uncond; cond]`` batch).  ``outputs`` holds what the transformer returned at every step of the last call."""

    def __init__(self, transformer, device='cpu', dtype=torch.bfloat16, seed=0, batch=1):
        self.transformer = transformer
        self.tokenizer = fd.FakeTokenizer()
        self.tokenizer_2 = FakeSentencePiece()
        self.vae_scale_factor = 8
        self.device, self.dtype, self.seed, self.batch = torch.device(device), dtype, seed, batch
        self.outputs, self.checked = [], []
        self.mask_fn = None                               # optional: (rows) -> an attention mask for every call
        self.rotary = True                                # False: image_rotary_emb=None
        self.table_layout = 'rows'                        # 'columns': the same f32 values, stored [d, rows] and passed transposed

    def check_inputs(self, prompt, prompt_2, *args, **kwargs):
        self.checked.append((prompt, prompt_2))

    def _randn(self, *shape, key):
        g = torch.Generator(device='cpu')
        g.manual_seed((self.seed * 1000003 + key) % (2 ** 31 - 1))
        return torch.randn(*shape, generator=g).to(self.dtype).to(self.device)

    def _table(self, h, w, d):
        tables = [torch.from_numpy(t).to(self.device) for t in R.flux_table(T5_ROWS, h, w, d)]
        if self.table_layout == 'columns':
            tables = [t.t().contiguous().t() for t in tables]
        return tuple(tables)

    def __call__(self, prompt, prompt_2=None, num_inference_steps=2, height=None, width=None, **kw):
        height, width = height or SIZE, width or SIZE
        self.check_inputs(prompt, prompt_2, height, width)
        h, w = height // CELL, width // CELL
        attn = self.transformer.transformer_blocks[0].attn
        dim = attn.inner_dim
        self.outputs = []
        with torch.no_grad():
            context = self._randn(self.batch, T5_ROWS, dim, key=7)
            rotary = self._table(h, w, dim // attn.heads) if self.rotary else None
            for step in range(num_inference_steps):
                hidden = self._randn(self.batch, h * w, dim, key=100 + step)
                mask = None if self.mask_fn is None else self.mask_fn(h * w + T5_ROWS)
                self.outputs.append(self.transformer(hidden, context, rotary, mask))
        return types.SimpleNamespace(images=['image-of:' + (prompt if isinstance(prompt, str) else prompt[0])])


def make_pipe(device='cpu', dtype=torch.bfloat16, seed=0, heads=2, dim_head=64, double=2, single=2, batch=1):
    state = torch.get_rng_state()
    torch.manual_seed(3000 + seed)
    try:
        model = FluxTransformer(heads, dim_head, double, single)
    finally:
        torch.set_rng_state(state)
    return FluxPipeline(model.to(device=device, dtype=dtype), device, dtype, seed, batch)


def record(pipe, on=True):
    """Start (or stop) recording what the softmax of every unmasked attention call saw; returns the list they are appended to."""
    calls = [] if on else None
    for block in list(pipe.transformer.transformer_blocks) + list(pipe.transformer.single_transformer_blocks):
        block.attn.record = calls
    return calls
