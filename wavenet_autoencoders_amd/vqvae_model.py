"""Drop-in ``VQVAE`` = Encoder + VectorQuantize + WaveNet (reference: vqvae_model.py:27-84) on the MI355X engine.

``state_dict`` keys: ``encoder.net.<i>.conv.{weight,bias}``, ``encoder.lin.{weight,bias}``, ``vq.embedding.weight``,
``wavenet.*`` -- the reference's, so its checkpoints load unchanged."""
import torch

from . import packing as P
from .wavenet_vocoder._base import ArenaModel, _leaf, check_saved, logits_grad_btc
from .wavenet_vocoder.wavenet import WaveNet, _ids_from_input, _start_classes, softmax_bct, stream_post


class _VQVAEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, c, gid, train, *params):
        eng = model.engine()
        if eng.g.vq == "plain":
            out = eng.forward(ids, c, gid, want_logits=True, train=train, dropout_on=model.training)
        else:
            out = eng.forward(ids, c, gid, want_logits=True, train=train, dropout_on=model.training, beta=model.beta,
                              vq_update=model.training)
        ctx.model, ctx.ids, ctx.gid = model, ids, gid
        ctx.gen, ctx.train = (eng.saved.gen if train else None), train
        eng.check_errors()     # IndexError for an id outside its table, like the reference's nn.Embedding (wavenet.py:185-187)
        return out["logits"], out["vq_loss"].reshape(()), out["perp"].reshape(())

    @staticmethod
    def backward(ctx, dy, dvq, dperp):
        from . import backward as BW
        model = ctx.model
        eng = model._engine
        if ctx.train:
            check_saved(eng, ctx.gen)
        dc = BW.decoder_backward(eng, ctx.ids, None, None, ctx.gid, None, ext_dy=logits_grad_btc(eng, dy))
        BW.frontend_backward(eng, dc, float(dvq) if dvq is not None else 0.0)
        BW.finish_grads(eng)
        _, views = model._grad_views(eng)
        return (None, None, None, None, None) + tuple(v.clone() for v in views)


class VQVAE(ArenaModel):
    """VQVAE(c_in, hid, K, wavenet, encoder_hid).forward(x, c, g, softmax=False) -> (y_hat, vq_loss, perp).
    quantizer: "plain" VectorQuantize (the reference's VQVAE), "sliced" SlicedVectorQuantize (num_slices slices, K1 codes in the
    second of two), "ema" VectorQuantizeEMA or "sliced_ema" SlicedVectorQuantizeEMA (vector_quantization.py:51-306) with their
    state_dict keys: vq.embedding{1..n}.weight, vq.ema_cluster_size[s], vq.ema_w[s].  The EMA kinds move their codebooks in every
    forward of a module in training mode (self.training, not the grad mode), and their codebooks get a zero gradient."""

    def __init__(self, c_in=39, hid=64, K=256, wavenet=None, encoder_hid=768, quantizer="plain", num_slices=2, K1=None, beta=0.25,
                 decay=0.99):
        super().__init__()
        self.beta = float(beta)
        if not isinstance(wavenet, WaveNet):
            raise TypeError("wavenet must be a wavenet_autoencoders_amd.wavenet_vocoder.WaveNet")
        wg = wavenet.geom
        if wg.Cc != hid:
            raise ValueError(f"wavenet.cin_channels ({wg.Cc}) must equal hid ({hid})")
        geom = P.Geometry(layers=wg.layers, stacks=wg.stacks, R=wg.R, G=wg.G, S=wg.S, O=wg.O, Cc=wg.Cc, Cg=wg.Cg, k=wg.k,
                          n_speakers=wg.n_speakers, upsample_scales=wg.upsample_scales, cin_pad=wg.cin_pad,
                          scalar_input=wg.scalar_input, use_speaker_embedding=wg.use_speaker_embedding, c_in=c_in,
                          encoder_hid=encoder_hid, K=K, conv_in=wg.conv_in, up_act=wg.up_act, up_act_slope=wg.up_act_slope,
                          output_distribution=wg.output_distribution, vq=quantizer, vq_slices=num_slices, K1=K1, vq_decay=decay)
        self.out_channels, self.scalar_input = wavenet.out_channels, wavenet.scalar_input
        self.dropout = float(getattr(wavenet, "dropout", 0.0))          # the decoder layers' dropout (modules.py:127-128)
        self._init_arena(geom, "")
        for name, shape in P.vq_buffer_specs(geom):                     # zeros, as the reference registers them
            m, leaf = _leaf(self, name)
            m.register_buffer(leaf, torch.zeros(shape))
        # keep the decoder's initial values (the reference builds the WaveNet first: vqwae_train.py:926-946)
        own = dict(self.named_parameters())
        for n, p in wavenet.named_parameters():
            own["wavenet." + n].data.copy_(p.data)

    def _params(self):
        params = dict(self.named_parameters())
        return [params[r] for r in self._pnames]

    def forward(self, x, c, g, softmax=False):
        ids = _ids_from_input(x, self.out_channels, self.scalar_input, self.engine())
        gid = g.reshape(-1) if g is not None else None
        params = self._params()
        train = torch.is_grad_enabled() and any(p.requires_grad for p in params)   # (inside Function.forward grad mode is off)
        train = train or (self.training and self.dropout > 0)                       # F.dropout follows module.training
        y, vq_loss, perp = _VQVAEFn.apply(self, ids, c.float(), gid, train, *params)
        if softmax:
            y = softmax_bct(y)
        return y, vq_loss, perp

    def incremental_forward(self, initial_input, c, g, T, softmax, quantize, tqdm, log_scale_min):
        """encoder -> VQ -> autoregressive decoder (vqvae_model.py:73-79)."""
        eng, args, kw, post = self._incremental_plan(initial_input, c, g, T, softmax, quantize, log_scale_min)
        with torch.no_grad():
            return post(eng.incremental_forward(*args, **kw))

    def incremental_stream(self, initial_input, c, g, T, softmax, quantize, tqdm, log_scale_min, chunk=1600):
        """incremental_forward in resumable launches: the encoder and the quantiser run once, on the whole `c` (they are not causal),
        then the decoder yields what incremental_forward returns `chunk` steps at a time (an int, or a sequence of chunk lengths
        summing to T; engine.incremental_stream) -- the same one-hot (B, C, n) / scalar (B, 1, n) shapes, the same bits given the same
        draws.  quantize=False feeds a vector back that stays on chip: ValueError."""
        eng, args, kw, post = self._incremental_plan(initial_input, c, g, T, softmax, quantize, log_scale_min)
        with torch.no_grad():
            return stream_post(eng.incremental_stream(*args, chunk, **kw), post)

    def _incremental_plan(self, initial_input, c, g, T, softmax, quantize, log_scale_min):
        """Encoder, quantiser and start classes, once; then as WaveNet._incremental_plan: (engine, (quant, gid, T), keyword arguments,
        post) with post: the engine's result dict (of the clip or of a chunk) -> the tensor the reference returns."""
        eng = self.engine()
        with torch.no_grad():
            if eng.weights_dirty:
                eng.prepare_weights()
            lat = eng.encoder_forward(c.float())
            quant, idx, stats = eng.vq_forward(lat)
            init = 127 if self.scalar_input else _start_classes(initial_input, self.out_channels, eng)     # one start class per utterance
        args = (quant, g.reshape(-1) if g is not None else None, int(T))
        if self.scalar_input:
            # the draws of the model's output distribution (wavenet.py:325-333): engine.incremental_forward makes them
            return eng, args, dict(mode="sample", log_scale_min=log_scale_min), lambda out: out["x"].unsqueeze(1)
        if quantize:
            if not softmax:
                raise ValueError("quantize=True draws from the softmax probabilities: pass softmax=True")
            return eng, args, dict(mode="sample", init_idx=init), lambda out: torch.nn.functional.one_hot(
                out["idx"].long(), self.out_channels).float().transpose(1, 2).contiguous()
        # quantize=False: the probability / logit rows are the outputs and the fed-back inputs (wavenet.py:303-305,335-338)
        return eng, args, dict(mode="probs" if softmax else "raw", init_idx=init), lambda out: out["logits"]

    def encode(self, x):
        """quantised latents of MFCC features (vqvae_model.py:80-84; inference_2019.py:243-262)."""
        eng = self.engine()
        with torch.no_grad():
            if eng.weights_dirty:
                eng.prepare_weights()
            lat = eng.encoder_forward(x.float())
            return eng.vq_forward(lat)[0]

    def encode_list(self, xs):
        """encode for a list of utterances of unequal lengths: xs, a sequence of (c_in, F_i) features -> a list of (hid, F_i') quantised
        latents, each bit for bit encode(x[None])[0] of that utterance alone, from one launch per encoder layer for the whole list
        (WaeEngine.encode_list; the reference has no list form -- zero-padding to one length changes the latents at the clip ends)."""
        with torch.no_grad():
            return [r["quant"] for r in self.engine().encode_list(xs, want_idx=False)]

    def forward_list(self, items, want_nll=True, want_stats=False, beta=0.25, quantize_channels=65536, log_scale_min=-7.0):
        """forward (no gradients, eval) for a list of utterances of unequal lengths: items, a sequence of mappings with `x` ((T_i,)
        class ids or scalars), `c` ((c_in, F_i) features) and `g` (a speaker id or None) -> (results, loss): per utterance dict(logits
        (out_channels, T_i), nll (T_i,) | None, nll_sum, count, quant, idx, latents) and the list's masked mean of the shifted
        cross-entropy (scalar inputs: of the mixture loss, with quantize_channels and log_scale_min).  Every utterance is bit for bit
        its own forward(x[None], c[None], g[None]) -- which a zero-padded batch is not at the utterance ends
        (WaeEngine.forward_list).  want_nll: on by default for every model.  want_stats: vq_loss, perp and hist per utterance besides."""
        its = [dict(x=it["x"], feats=it["c"], gid=it.get("g")) for it in items]
        with torch.no_grad():
            return self.engine().forward_list(its, want_nll=bool(want_nll), want_stats=want_stats, beta=beta,
                                              quantize_channels=quantize_channels, log_scale_min=log_scale_min)

    def score_list(self, items, beta=0.25, quantize_channels=65536, log_scale_min=-7.0):
        """What forward returns besides the logits -- loss, vq_loss, perplexity -- for a list of utterances of unequal lengths, per
        utterance and for the list as one batch (WaeEngine.score_list): items as forward_list -> (results, totals), totals a dict of
        0-d tensors ce, vq_loss, perp, loss = ce + vq_loss, count, frames; every dict of results carries nll, nll_sum, count, vq_loss,
        perp and hist (how often the utterance used every code)."""
        its = [dict(x=it["x"], feats=it["c"], gid=it.get("g")) for it in items]
        with torch.no_grad():
            return self.engine().score_list(its, beta=beta, quantize_channels=quantize_channels, log_scale_min=log_scale_min)

    def encode_session(self, want_latents=False, window=None):
        """encode for utterances whose features still arrive: WaeEngine.encode_session (open / feed_list / end), whose `quant` chunks,
        concatenated per utterance, are bit for bit encode_list([x])[0].  window: the session in constant memory (rings of `window`
        feature frames per open utterance), the same bits."""
        return self.engine().encode_session(want_latents=want_latents, window=window)
