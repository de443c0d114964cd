"""SDEDecoder -- MI355X path of models/decoders/dec_hivt_nusargo_sde.py:14-105: fuse local+global
embeddings into y0 [K*N,64], Euler-Maruyama over the future grid with learned drift and
scalar-broadcast diffusion (Euler-Maruyama or Milstein), heads -> loc/scale/pi.

`method: euler` (the shipped one) or `method: milstein` (torchsde's MilsteinIto: the same fixed-step schedule and noise, plus the
column-sum gdg term of the scalar-broadcast diffusion; trained through the Milstein backward, whose reverse sweep differentiates
that term as torchsde's create_graph vjp does).
Constructor kwargs as in configs/nusargo/hivt_nuSArgo_sdesepenc_sdedec.yml:64-76; call signature
`decoder(data=..., local_embed=..., global_embed=...) -> {'loc','pi','reg_mask'}`; `uncertain: False` (DEC:56, DEC:100-101):
no `scale.*` parameters and `loc` [K, N, T, 2] -- the kernels run with a zero stand-in head and the scale channels are dropped.
"""
from typing import Optional

from trajsde_amd.models.params import ParamTree
from trajsde_amd import runtime, stage_autograd
from trajsde_amd.schedule import ITO_METHODS, SDE_METHODS


def check_method(method):
    """the decoder's `method` kwarg, handed to stock torchsde.sdeint (DEC:88): `euler` and `milstein` are built (MilsteinIto with
    its default grad_free=False; csrc/decoder.hip); everything else is refused the way torchsde would, or as not built"""
    if method is None:
        raise NotImplementedError("method=None: torchsde then picks srk for this Ito SDE with diagonal noise, which is not built "
                                  "(srk needs the space-time Levy area, a second random stream the Philox noise model does not have)")
    if method not in SDE_METHODS:
        raise ValueError(f"Expected method in {SDE_METHODS}, but found {method}.")
    if method not in ITO_METHODS:
        raise ValueError(f"method {method!r} is a Stratonovich solver: torchsde does not accept it for this Ito SDE")
    if method == "srk":
        raise NotImplementedError("method='srk' is not built: it needs the space-time Levy area, a second random stream the Philox "
                                  "noise model does not have (built: euler, milstein)")
    return method


class SDEDecoder(ParamTree):
    last_support_status = None

    def __init__(self, **kwargs) -> None:
        super().__init__()
        self.set_init_seed(kwargs.pop("init_seed", None))
        for key, value in kwargs.items():
            setattr(self, key, value)
        self.input_size, self.hidden_size = self.global_channels, self.local_channels
        d = self.hidden_size
        if d != 64 or self.input_size != 64:
            raise NotImplementedError("kernels are specialised for 64 channels (CFG:64-76)")
        self.method = check_method(getattr(self, "method", None))
        stage_autograd.check_decoder(self)                       # `autograd: true`: Euler-Maruyama and the scale head only
        self.linear("aggr_embed.0", d, self.input_size + d)
        self.layernorm("aggr_embed.1", d)
        self.sde_nets("lsde_func", d, ("g_func",))
        self.head("decoder", d, d, 2)
        if self.uncertain:
            self.head("scale", d, d, 2)
        else:                                                    # DEC:56: no scale head; 'loc' is [K, N, T, 2] (DEC:100-101)
            self.absent_head("scale", d, d, 2)
        self.head("pi", d + self.input_size, d, 1)
        self.token("hidden", d)                                  # present in checkpoints, unused (DEC:69)
        self.set_init_seed(None)
        self._rt = runtime.StageRuntime(self, "decoder")

    def forward(self, data, local_embed, global_embed, noise: Optional["runtime.NoiseSpec"] = None):
        """With `autograd: true` among the kwargs, and an input or a parameter requiring grad while grad mode is on, `loc` and `pi` come
        from the stage's autograd node (stage_autograd.DecoderNode), whose backward is the cotangent route over `cotangent_support:
        all` (default) or `winner` paths; `winner` leaves its status words on `self.last_support_status`."""
        if stage_autograd.active(self, local_embed, global_embed):
            return stage_autograd.decoder(self, data, local_embed, global_embed, noise)
        return self._rt.decoder_forward(data, local_embed, global_embed, noise)

    def sample(self, data, local_embed, global_embed, n_samples: int, noise: Optional["runtime.NoiseSpec"] = None,
               sample_stride: Optional[int] = None, return_samples: bool = False):
        """Monte-Carlo decoding: `n_samples` sample paths of every (mode, actor) from these embeddings in one launch, reduced on the
        device -> {'loc' (sample 0: what forward() returns under the same noise), 'pi', 'reg_mask', 'loc_mean', 'loc_cov'[, 'samples']}
        (runtime.StageRuntime.decoder_forward_mc).  Inference only: eval mode, no gradients."""
        if self.training:
            from trajsde_amd import _lib
            raise _lib.TrajsdeError("SDEDecoder.sample is inference only: call model.eval() first")
        return self._rt.decoder_forward_mc(data, local_embed, global_embed, n_samples, noise=noise, sample_stride=sample_stride,
                                           return_samples=return_samples)
