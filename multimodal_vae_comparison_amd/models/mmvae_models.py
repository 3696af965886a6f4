"""The multimodal mixers behind the reference's registry names (reference: models/mmvae_models.py).

`objective()` is the per-step hot path: towers -> ONE fused latent kernel (product of experts, reparameterised
samples, analytic KL rows) -> decoders -> fused per-sample reconstruction sums -> ONE ELBO assembly kernel.
No host synchronisation anywhere (the reference forces >= 6 per step)."""
import os
from itertools import chain, combinations

import torch
import torch.distributions as dist

from .. import ops
from .mmvae_base import TorchMMVAE, normal, packed_head
from .objectives import recon_rowsum


class MoPOE(TorchMMVAE):
    """Generalised multimodal ELBO (mmvae_models.py:253-410).

    Parity-critical behaviour of the reference kept as is (SURVEY Appendix B + tests/golden):
      * the subset posteriors are stacked as (n_subsets, 1, B, D), so `mixture_component_selection`
        (mmvae_models.py:396-410) splits the SINGLETON axis: the joint posterior is the LAST subset -- the product
        of all modality experts and the N(0,1) prior expert -- for every sample;
      * encoder "logvar" = softmax + 1e-6 is used as log-variance inside the product and as sigma in Normal();
        the product returns the variance, used as sigma; one independent z per modality from the same joint;
      * KL terms: q_m = N(mu_m, sigma = lv_m) and the joint, against N(0, softmax(theta) * D), weights 1/(M+1).
    """

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        super().__init__(vaes, n_latents, **obj_config)
        self.model_config = model_config
        self.modelName = "mopoe"
        self._require_normal_priors()
        self.subsets = self.set_subsets()
        self.weights = None

    def set_subsets(self):
        """mmvae_models.py:279-294: non-empty subsets in itertools.combinations order, keyed 'mod_i_mod_j'"""
        xs = list(self.vaes.keys())
        subsets = {}
        for mod_names in chain.from_iterable(combinations(xs, n) for n in range(len(xs) + 1)):
            subsets["_".join(sorted(mod_names))] = [self.vaes[m] for m in sorted(mod_names)]
        subsets.pop("", None)
        return subsets

    # ---- hot path --------------------------------------------------------------------------------
    def _elbo_weights(self, B):
        """rows of the ELBO assembly (loss, kld) over [M recon rows, M+1 KL rows] (weighted_group_kld, objectives.py:184-201)"""
        names = list(self.vaes.keys())
        M = len(names)
        w_kl = 1.0 / (M + 1)
        lam = [float(self.vaes[n].llik_scaling) for n in names]
        return [[l / B for l in lam] + [self.obj_fn.beta * w_kl / B] * (M + 1),
                [0.0] * M + [w_kl / B] * (M + 1)]

    def _elbo_terms(self, mods, seeds=None):
        """Forward pass up to the per-row ELBO terms (mmvae_models.py:296-320 + weighted_group_kld,
        objectives.py:184-201): returns (recs, kl, W, streams, device) and leaves the tower streams un-joined.

        Stream choreography (every cross-stream wait costs ~9 us at this kernel size, a wait whose event has already
        fired costs nothing): tower i encodes on stream i; the fusion kernel runs on the LAST tower's stream -- the
        text encoder, the longer of the two -- after that stream has waited for the others; the decoders then rotate
        by one stream, so modality 0's decoder (the image ConvT stack, the longer one) continues on the fusion stream
        without a wait.  autograd replays every node on its forward stream, so the backward pass mirrors this."""
        self._begin_step()
        names = list(self.vaes.keys())
        M = len(names)
        dev = next(v["data"] for v in mods.values() if v["data"] is not None).device
        # (which tower keeps the capture stream, and the capture order of the towers, decide how hipGraph partitions the
        # step into queues: measured, see DESIGN.md section 5 -- tower 0 on the capture stream, captured first)
        streams = self._tower_streams(dev)
        cur = torch.cuda.current_stream(dev)
        real = [cur if st is None else st for st in streams]
        self._fork(streams, dev, mods)
        B, D = next(v["data"] for v in mods.values() if v["data"] is not None).shape[0], self.n_latents
        W = self._elbo_weights(B)
        # the M rsamples (:363-369): drawn by the fusion kernel itself unless the noise is replayed (`eps_override`)
        eps = None
        enc = [None] * M
        for i, (n, st) in enumerate(zip(names, streams)):
            with torch.cuda.stream(st):
                tower = self.vaes[n].enc
                tower.raw_heads = True      # lv = softmax(u) + eta is applied by the fused latent kernel
                ops.Marks.mark(f"enc {n} start")
                try:
                    mu_lv = tower(mods[n])
                finally:
                    tower.raw_heads = False
                enc[i] = tuple(ops.mark_tensor(t, f"enc {n} out[{j}]") for j, t in enumerate(mu_lv))
                if i == 0 and self.eps_override is not None:
                    # one replayed rsample per modality (:363-369), behind tower 0's encoder: that stream idles until the
                    # fusion anyway
                    eps = self._draw_many(M, B, D, dev)
        # the fusion runs on the last tower's stream, the decoders rotate by one stream.  (Round 6,
        # re-measured with the shorter text chain: fusion + every decoder on its OWN tower's stream -- no cross-stream wait
        # on the image chain in either direction -- replays at 0.490 ms against 0.388: hipGraph serialises that layout.)
        self._fuse_stream = fuse = real[-1]
        theta = self._pz_params[1]
        # every tower's heads (tower 0's with the replayed noise drawn behind them) cross to the fusion's stream
        for i, st in enumerate(real):
            ops.StreamPlan.hand(list(enc[i]) + (list(eps or []) if i == 0 else []), fuse, after=st)
        with torch.cuda.stream(fuse):
            packed = [packed_head(mu, lv) for mu, lv in enc]
            if seeds is not None and getattr(self, "early_adam", None) is not None and ops.GradReducer.defer_next:
                packed[-1] = ops.EarlyStepPoint.apply(packed[-1])      # (its tower's stream IS the fusion's)
            if eps is None:
                _, kl, z = ops.poe_reparam_kl(theta, packed, M, True, (1 << (M + 1)) - 1, theta.grad, raw=True,
                                              rng=self._rng_state)
            else:
                _, kl, z = ops.poe_reparam_kl(theta, packed, eps, True, (1 << (M + 1)) - 1, theta.grad, raw=True)
        ops.StreamPlan.hand([kl], cur)
        order = [(i, names[i], real[(i + M - 1) % M]) for i in range(M)]
        for i, _, st in order:      # (all of them before the first decoder is queued: none waits for another's launches)
            ops.StreamPlan.hand([z[i]], st, after=fuse)
        recs = [None] * M
        # (the stream of a decoder that does not share the fusion's: idle behind that decoder's backward pass)
        self._idle_stream = next((st for _, _, st in reversed(order) if st != fuse), None)
        for i, n, st in order:
            vae = self.vaes[n]
            with torch.cuda.stream(st):
                zi = ops.mark_tensor(z[i], f"dec {n} z")
                if seeds is not None and getattr(self, "early_adam", None) is not None and ops.GradReducer.defer_next:
                    zi = ops.DecoderEnd.apply(zi)           # (parked weight gradients of this decoder: out before the fusion)
                if seeds is not None and st != fuse and ops.GradReducer.side_head is not None:
                    zi = ops.StreamIdlePoint.apply(zi)      # (this decoder's stream idles behind its backward pass)
                if seeds is not None:      # the term's upstream gradient is known: its kernel also writes its backward
                    with ops.ConstSeed(seeds[i], W[0][i]):
                        # (a bce decoder is handed its target: Dec_CNN then folds the loss into its last layer's launch)
                        fold = vae.ltype == "bce" and mods[n]["masks"] is None
                        out, _ = vae.dec({"latents": zi.unsqueeze(0), "masks": mods[n]["masks"],
                                          "bce_target": mods[n]["data"] if fold else None})
                        r = recon_rowsum(vae.ltype, out, mods[n], laplace=self._lap(vae))
                else:
                    out, _ = vae.dec({"latents": zi.unsqueeze(0), "masks": mods[n]["masks"]})
                    r = recon_rowsum(vae.ltype, out, mods[n], laplace=self._lap(vae))
                recs[i] = ops.mark_tensor(r, f"dec {n} recon")   # (B,) = -lpx_z / llik_scaling
            ops.StreamPlan.hand([recs[i]], cur)      # (joined by objective() / finish_step())
        self._fusion_inputs = packed        # the towers' packed head outputs: where the backward can be cut in two
        return recs, kl, W, streams, dev

    def objective(self, mods):
        recs, kl, W, streams, dev = self._elbo_terms(mods)
        self._join(streams, dev)
        ops.Marks.mark("joined decoders")
        out = ops.lincomb_rows(recs + [kl], W)                              # rows: M recon sums, M+1 KL rows
        return {"loss": out[0], "kld": out[1], "reconstruction_loss": recs}

    def backward_encoders(self):
        """second half of objective_backward(mods, cut=True): the encoders' backward from the saved head gradients"""
        hs, dhs, streams, dev = self._cut
        self._cut = None
        for st in streams:           # the towers' weight-gradient kernels run on their streams: the fold must join them
            if st is not None:
                ops.GradReducer.note_stream(dev, st)
        torch.autograd.backward(hs, list(dhs))
        self._join(streams, dev)

    def objective_backward(self, mods, cut=False):
        """objective(mods)["loss"].backward() without the join in the middle: the loss is LINEAR in the per-row terms
        (recs, kl) with host-side constant weights, so every tower's backward is seeded with those constants as soon as
        its own forward is done -- no tower waits for the other one's decoder or for the loss kernel.  The loss values
        are assembled afterwards, off the critical path.  Used by the captured training step (trainer.capture)."""
        first = next(v["data"] for v in mods.values() if v["data"] is not None)
        B, dev, M = first.shape[0], first.device, len(self.vaes)
        W = self._elbo_weights(B)
        key = (tuple(W[0]), B, str(dev))
        if getattr(self, "_seed_key", None) != key:      # persistent: their addresses identify them in backward
            self._seeds = [torch.full((B,), W[0][i], device=dev) for i in range(M)]
            self._seeds.append(torch.tensor(W[0][M:], device=dev).reshape(-1, 1).expand(M + 1, B).contiguous())
            self._seed_key = key
        recs, kl, W, streams, dev = self._elbo_terms(mods, self._seeds)
        def assemble(stream):
            with torch.cuda.stream(stream), torch.no_grad():
                return ops.lincomb_rows([r.detach() for r in recs] + [kl.detach()], W)

        out = None
        # the logged values ride on the end-of-backward fold launch (one extra workgroup): the forward's row sums are long
        # finished by then, and a launch of their own would sit between the fold and the optimiser (assembling them on a
        # side stream instead cost +20 us: DESIGN section 5)
        tail = ops.GradReducer.tail = ops.lincomb_rows_args(recs + [kl], W)
        early = getattr(self, "early_adam", None)
        if early is not None and not cut and ops.GradReducer.defer_next:
            # (captured one-GPU step) the decoders' + prior's parameters are updated as soon as the tower that shares the
            # fusion's stream has queued its last backward launch: ops.GradReducer.run_early_step
            ops.GradReducer.early_step = (early[0], self._fuse_stream, early[1], early[2])
            ops.GradReducer.dw_open = True
        if not cut and ops.GradReducer.defer_next and self._idle_stream is not None and M == 2:
            # (captured one-GPU step of two towers, the layout this was measured in) the image decoder's large conv weight
            # gradients leave its backward chain
            ops.GradReducer.cw_streams = (self._fuse_stream, self._idle_stream)
        if cut:
            # decoders + fusion only: the gradients of the towers' head outputs come back instead of flowing on
            self._cut = (list(self._fusion_inputs), torch.autograd.grad(recs + [kl], self._fusion_inputs, self._seeds),
                         streams, dev)
        else:
            torch.autograd.backward(recs + [kl], self._seeds)
        ops.GradReducer.tail = ops.GradReducer.early_step = None
        ops.GradReducer.dw_open = ops.GradReducer.early_ready = False
        ops.GradReducer.cw_streams = None
        if tail is not None and tail["done"]:
            out = tail["args"][2].unbind(0)
        if out is None:
            self._join(streams, dev)
            out = assemble(None)
        self._unjoined = (streams, dev)
        return {"loss": out[0], "kld": out[1], "reconstruction_loss": recs}

    def finish_step(self):
        """join the streams objective_backward() left running (call after the optimiser step has been queued)"""
        pending, self._unjoined = getattr(self, "_unjoined", None), None
        if pending is not None:
            self._join(*pending)

    # ---- API surface (inference / evaluation) ------------------------------------------------------
    def modality_mixing(self, input_batch):
        """mmvae_models.py:322-349"""
        latents = {}
        enc_mods = self.encode(input_batch)
        latents["modalities"] = enc_mods
        distr_subsets, last = {}, None
        n_all = len(self.vaes)
        for s_key, mods in self.subsets.items():
            if all(m.modelName in input_batch and input_batch[m.modelName]["data"] is not None for m in mods):
                mus = [enc_mods[m.modelName]["shared"][0] for m in mods]
                lvs = [enc_mods[m.modelName]["shared"][1] for m in mods]
                s_mu, s_var = self.product_of_experts(mus, lvs, with_prior=(len(mods) == n_all))   # :385-389
                distr_subsets[s_key] = [s_mu.unsqueeze(0), s_var.unsqueeze(0)]
                last = (s_mu, s_var)
        self.weights = (1 / float(len(distr_subsets))) * torch.ones(len(distr_subsets), device=last[0].device)
        latents["joint"] = [last[0], last[1]]        # singleton-axis selection => last available subset (:396-410)
        latents["subsets"] = distr_subsets
        return latents

    def _proposal_size(self, n_given):
        return 2 ** n_given - 1

    def _proposal(self, mods, given):
        """every non-empty subset of `given`: the subset products modality_mixing() builds (the prior expert joins the
        subset of ALL modalities only), (mu, variance used as scale)"""
        subsets = self.modality_mixing(self._given_only(mods, given))["subsets"]
        comps = torch.stack([torch.cat([mu[0], var[0]], -1) for mu, var in subsets.values()])
        return comps, [False] * comps.shape[0]

    def _sample(self, x, K=1, of=None):
        """K draws per modality from the joint, in modality order, each taken when its modality is read (every modality's
        draw is taken whichever one `of` asks for)"""
        latents = self.modality_mixing(x)
        j_mu, j_var = latents["joint"]
        return latents, ((mod, j_mu + j_var * self._draws(K, *j_mu.shape, j_mu.device)) for mod in self.vaes)

    def _unimodal(self, head):
        return {m: (*q["shared"], dist.Normal) for m, q in head["modalities"].items() if q["shared"] is not None}

    def forward(self, inputs, K=1):
        """mmvae_models.py:351-370"""
        latents, zs = self._sample(inputs, K)
        qz_d, px_d, z_d, qz_joint = {}, {}, {}, {}
        for mod, z in zs:
            vae = self.vaes[mod]
            sh = latents["modalities"][mod]["shared"]
            qz_d[mod] = normal(*sh) if sh is not None else None
            qz_joint[mod] = normal(*latents["joint"])
            z_d[mod] = {"latents": z, "masks": inputs[mod]["masks"]}
            px_d[mod] = self._px(vae, *vae.dec(z_d[mod]))
        return self.make_output_dict(qz_d, px_d, z_d, qz_joint)


class POE(TorchMMVAE):
    """MVAE, product of experts (mmvae_models.py:134-250)."""

    # decoder calls of one step spread over the two streams by their launch counts (_decoder_lanes); MMVAE_POE_BALANCE=0:
    # every call on its tower's stream
    balance_decoder_calls = os.environ.get("MMVAE_POE_BALANCE", "1") != "0"

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        super().__init__(vaes, n_latents, **obj_config)
        self.model_config = model_config
        self.modelName = "poe"
        for vae in self.vaes.values():
            assert vae.prior_str in ["normal", "gaussian"], "POE only works with gaussian priors! Adjust the config"
        # utils.subsample_input_modalities (utils.py:86-112) iterates a Python set => its order within one subset
        # size depends on PYTHONHASHSEED; the default here is itertools order, `subset_order` pins another one.
        self.subset_order = None
        self.batch_dropout_towers = True      # decoders with dropout: all subset passes in one call (objective docstring)
        self._job_calls = {}                  # launches of a decoder call the last time it ran (_decoder_lanes)

    def _subsets(self):
        names = list(self.vaes.keys())
        if self.subset_order is not None:
            return [tuple(names[i] for i in s) for s in self.subset_order]
        return [c for n in range(1, len(names) + 1) for c in combinations(names, n)]

    def objective(self, mods):
        """mmvae_models.py:159-187: sum over input subsets of -(sum_b sum_m lpx - beta sum_b KL(joint || prior)).

        The reference runs the whole model once per subset (2^M - 1 passes: every encoder 2^(M-1) times on the SAME
        input, every decoder 2^M - 1 times).  Round 4: a tower without dropout (the CNN image towers; any tower in eval
        mode) takes all of its passes in ONE call -- the encoder's output is simply shared by the subsets it belongs to,
        the decoder decodes the (n_subsets * B) latent samples as one batch and the row-sum kernels pair output row r with
        target row r % B.  Same sums, same noise draws in the same order.  Decoders WITH dropout do the same
        (`batch_dropout_towers`: their masks are then drawn once for all passes); encoders with dropout keep one call per
        subset -- the text encoder's positional encoding is indexed by the BATCH position (nn_modules.py:430-438), which a
        repeated batch would change.  BASELINE configs[0]: 181 -> 96 C-ABI calls per step."""
        self._begin_step()
        names = list(self.vaes.keys())
        M = len(names)
        theta = self._pz_params[1]
        subsets = self._subsets()
        NS = len(subsets)
        dev = next(v["data"] for v in mods.values() if v["data"] is not None).device
        streams = self._tower_streams(dev)

        def one_call(part):      # every pass of this tower gives the same function of its input
            return getattr(part, "drop_state", None) is None or not part.training

        # ---- encoders: packed[s][n] for n in subset s ----
        packed = [dict() for _ in subsets]
        raw_heads = dev.type == "cuda" and all(hasattr(v.enc, "raw_heads") and v.enc.enc_mu_logvar for v in self.vaes.values())
        def encode(n, st):
            member = [s for s, S in enumerate(subsets) if n in S]
            enc = self.vaes[n].enc
            # lv = softmax(u) + eta is applied by the fusion kernels (as MoPOE._elbo_terms does): no softmax launch
            # behind the heads, none in front of their backward
            enc.raw_heads = raw_heads
            try:
                if one_call(enc):
                    p = packed_head(*enc(mods[n]))
                    for s in member:
                        packed[s][n] = p
                elif self.batch_dropout_towers and len(member) > 1 and getattr(enc, "takes_repeat", False) and \
                        enc.repeat_ok(mods[n]):
                    # an encoder WITH dropout whose passes differ only in their masks: all of them as one call over
                    # len(member) * B sequences (round 5: the text encoder's positional term follows the sample's
                    # position in the ORIGINAL batch, ops.embed_pe), rows k * B + b
                    p = packed_head(*enc(dict(mods[n], repeat=len(member))))
                    for s, part in zip(member, ops.split_rows(p, len(member))):      # (row blocks; ONE cat in backward)
                        packed[s][n] = part
                else:
                    for s in member:
                        packed[s][n] = packed_head(*enc(mods[n]))
            finally:
                enc.raw_heads = False
            return [packed[s][n] for s in member]
        # Tensors that cross streams (a tower's heads -> the fusion; the latent samples -> decoder calls on the other stream;
        # their row sums -> the ELBO assembly) are handed to the consuming stream (_tower_phase).  Without it the allocator
        # hands a block out again as soon as the host drops the last reference -- found in round 6 in the CAPTURED step: the
        # image-only subset's z (capture stream) was re-used by the image decoder's backward while the text decoder's
        # cross-attention weight gradient, queued long before on the side stream, had yet to read it.
        self._tower_phase(zip(names, streams), encode, dev, batch=mods)
        # ---- fusion per subset (one noise draw each, in subset order) ----
        zs, kl_blocks = [], []
        D = self.n_latents
        B = next(iter(packed[0].values())).shape[0]
        draws = self._draw_many(NS, B, D, dev)      # (one launch; `eps_override`: NS recorded draws in subset order)
        for s, S in enumerate(subsets):
            ps = [packed[s][n] for n in names if n in S]
            eps = [draws[s]]
            E = len(ps)
            _, kl, z = ops.poe_reparam_kl(theta, ps, eps, True, 1 << E, theta.grad, raw=raw_heads)
            zs.append(z[0])
            kl_blocks.append(kl)             # (E + 1, B): the joint's KL is the last row
        # ---- decoders: one (passes, B) block of row sums per call ----
        # One call for all passes of a decoder that run under the SAME mask: the B-row latent samples of those subsets are
        # one batch (row k * B + b).  Subsets that contain the modality decode under its mask, the others under `masks=None`
        # (the decoder's full-length all-ones mask, another sequence length for the text tower): two groups.
        # optimal_sigma fits ONE sigma per call, so its passes cannot share one.  A decoder WITH dropout then draws its
        # masks once per group instead of per pass (independent masks either way; the extracted-mask parity test splits
        # them by pass).
        jobs = []      # (modality index, name, subsets of the call, mask of the call, (slot, call) of its dropout state)
        for i, n in enumerate(names):
            vae = self.vaes[n]
            mk = mods[n]["masks"]
            share = vae.ltype != "optimal_sigma" and (one_call(vae.dec) or self.batch_dropout_towers)
            groups = [[s_ for s_, S in enumerate(subsets) if n not in S], [s_ for s_, S in enumerate(subsets) if n in S]]
            if mk is None:
                groups = [list(range(NS))]
            groups = sorted([g for g in groups if g], key=lambda g: g[0])          # call order = first member's order
            for g in groups:
                gm = mk if (mk is not None and n in subsets[g[0]]) else None
                for part in ([g] if share and len(g) > 1 else [[s_] for s_ in g]):
                    jobs.append((i, n, part, gm))
        lanes = self._decoder_lanes(jobs, streams, B)
        # every call's input batch -- the samples of its subsets as row blocks -- from ONE launch, and in backward every
        # sample's gradient as one sum over the calls that decoded it (ops.RowsFan), instead of a torch.cat per call and an
        # addition per sample
        plan = [(len(g), D, [(s_, k, 0) for k, s_ in enumerate(g)]) for _, _, g, _ in jobs]
        z_ins = ops.rows_fan(plan, zs) if (zs[0].is_cuda and ops.RowsFan.supported(plan, zs)) else None
        rec_blocks = []

        def decode(j_, st):
            (i, n, g, gm), begun = jobs[j_], lanes[j_][1]
            vae = self.vaes[n]
            c0 = ops.CALLS[0]
            m_in = gm if (gm is None or len(g) == 1) else gm.repeat(len(g), 1)
            if z_ins is not None:
                z_in = z_ins[j_]
            else:
                z_in = torch.cat([zs[s_] for s_ in g], 0) if len(g) > 1 else zs[g[0]]
            job = {"latents": z_in.unsqueeze(0), "masks": m_in}
            if begun is not None:
                job["drop_begun"] = begun
            if gm is None and mods[n]["masks"] is not None and getattr(vae.dec, "takes_keep_steps", False):
                job["keep_steps"] = int(mods[n]["masks"].shape[1])      # (recon_rowsum slices to the target's mask length)
            out, _ = vae.dec(job)
            r = recon_rowsum(vae.ltype, out, mods[n])                    # target row = output row % B
            rec_blocks.append((r.view(len(g), B), i, list(g)))           # the call's rows as ONE (passes, B) block
            self._job_calls[(n, len(g), gm is None, B)] = ops.CALLS[0] - c0
            return r
        self._tower_phase([(j_, st) for j_, (st, _) in enumerate(lanes)], decode, dev, reads=z_ins or zs, batch=mods)
        # ELBO assembly straight on the calls' row BLOCKS (round 5: slicing the batched row sums and selecting the joint KL
        # row cost ~40 ATen fill / copy / add launches per step in forward + autograd): every block is addressed in place,
        # a row that does not enter an output has weight 0.  Outputs: loss, kld and -- while they fit (<= 4 outputs) -- the
        # logged per-modality reconstruction sums of each modality's own singleton subset (mmvae_models.py:181-182).
        blocks, W_loss, W_kld = [], [], []
        W_ind = [[] for _ in range(M)]
        n_rows = sum(b.shape[0] for b, _, _ in rec_blocks) + sum(k.shape[0] for k in kl_blocks)
        whole_kl = n_rows <= 32
        for blk, i, subs in rec_blocks:
            blocks.append(blk)
            for s_ in subs:
                W_loss.append(float(self.vaes[names[i]].llik_scaling))
                W_kld.append(0.0)
                for j in range(M):
                    W_ind[j].append(1.0 if (j == i and s_ == i) else 0.0)
        for s_, kl in enumerate(kl_blocks):
            E1 = kl.shape[0]
            if whole_kl:
                blocks.append(kl)
                W_loss += [0.0] * (E1 - 1) + [float(self.obj_fn.beta)]
                W_kld += [0.0] * (E1 - 1) + [1.0 / NS]
                for j in range(M):
                    W_ind[j] += [0.0] * E1
            else:
                blocks.append(kl[E1 - 1])
                W_loss.append(float(self.obj_fn.beta))
                W_kld.append(1.0 / NS)
                for j in range(M):
                    W_ind[j].append(0.0)
        if M <= 2 and len(W_loss) <= 32:
            out = ops.lincomb_rows(blocks, [W_loss, W_kld] + W_ind)
            ind = [o.detach() for o in out[2:]]
        else:
            out = ops.lincomb_rows(blocks, [W_loss, W_kld])
            ind = [None] * M
            for blk, i, subs in rec_blocks:
                for k, s_ in enumerate(subs):
                    if s_ == i:
                        ind[i] = blk[k].detach().sum()
        return {"loss": out[0], "reconstruction_loss": ind, "kld": out[1]}

    def _decoder_lanes(self, jobs, streams, B):
        """Stream of every decoder call of a step, [(stream, (slot, call) | None)] in call order.

        By default a call runs on its tower's stream.  Two streams, several calls: the calls are spread over the two by the
        number of launches each one took the last time it ran (longest first onto the shorter lane) -- BASELINE configs[0]
        decodes the text once at full length for the image-only subset (45 steps: the layer's launch-per-op form, ~20
        launches each way) and once under the mask for the other two (one launch per layer); behind one another on the text
        tower's stream they are the step's critical chain while the image decoder's stream idles.  A decoder with dropout
        whose calls leave its tower's stream gets its per-call counter advances up front, in call order, on the caller's
        stream (DropoutState.begin launches on the current stream: two lanes would race on the counter)."""
        own = [(streams[i], None) for i, _, _, _ in jobs]
        self.decoder_calls_moved = 0      # (tests: calls of the last step that left their tower's stream)
        lanes = sorted(set(streams), key=lambda s: s is not None)
        if not POE.balance_decoder_calls or len(lanes) != 2 or len(jobs) < 3:
            return own
        cost = [self._job_calls.get((n, len(g), gm is None, B)) for i, n, g, gm in jobs]
        if any(c is None for c in cost):
            return own
        load = {lanes[0]: 0, lanes[1]: 0}
        pick = [None] * len(jobs)
        for k in sorted(range(len(jobs)), key=lambda k: -cost[k]):
            st = min(lanes, key=lambda s: (load[s], s is not None))
            pick[k] = st
            load[st] += cost[k]
        out = []
        for k, (i, n, g, gm) in enumerate(jobs):
            dec = self.vaes[n].dec
            ds = getattr(dec, "drop_state", None)
            moved = any(pick[j] is not streams[i] for j, job in enumerate(jobs) if job[0] == i)
            begun = ds.begin() if (ds is not None and dec.training and moved) else None
            out.append((pick[k], begun))
            self.decoder_calls_moved += pick[k] is not streams[i]
        return out

    prior_expert = True      # the N(0, 1) expert joins the product (MVTCAE: it does not)

    def modality_mixing(self, x):
        """mmvae_models.py:210-232: prior expert + present encoders -> product"""
        mus, lvs, single = [], [], {}
        for m, vae in self.vaes.items():
            if x[m]["data"] is not None:
                mu, lv = vae.enc(x[m])
                single[m] = normal(mu, lv)
                mus.append(mu)
                lvs.append(lv)
        mu, var = self.product_of_experts(mus, lvs, with_prior=self.prior_expert)
        return mu, var, single

    def _proposal_size(self, n_given):
        return 1

    def _proposal(self, mods, given):
        """the product of the prior expert and the experts of `given` (modality_mixing), (mu, variance used as scale)"""
        mu, var, _ = self.modality_mixing(self._given_only(mods, given))
        return torch.cat([mu, var], -1).unsqueeze(0), [False]

    def _sample(self, x, K=1, of=None):
        """K draws from the product, shared by every modality"""
        mu, var, single = self.modality_mixing(x)
        z = mu + var * self._draws(K, *mu.shape, mu.device)
        return (normal(mu, var), single), [(mod, z) for mod in x]

    def _unimodal(self, head):
        return {m: (q.loc, q.scale, dist.Normal) for m, q in head[1].items()}

    def _joint_posterior(self, head):
        return head[0].loc, head[0].scale

    def forward(self, inputs, K=1):
        """mmvae_models.py:189-208"""
        (qz_x, single), zs = self._sample(inputs, K)
        z_d = {key: {"latents": z, "masks": inputs[key]["masks"]} for key, z in zs}
        px_d = {mod: normal(*vae.dec(z_d[mod])) for mod, vae in self.vaes.items()}
        return self.make_output_dict(single, px_d, z_d, joint_dist={key: qz_x for key in z_d})


class MVTCAE(POE):
    """MVTCAE, total-correlation objective (Hwang et al., NeurIPS 2021; not in the reference: a plugin on the base class's
    contract).  Joint = product of the PRESENT experts without a prior expert; one z per step, every modality decoded once
    from it.  With M modalities, r_m the reconstruction row sums (the sign POE gives them), kl[M] = KL(joint || prior) and
    kl[e] = KL(joint || q_e) -- the conditional terms that pull the joint towards every unimodal posterior:

        loss = sum_b [ (M - alpha) / M sum_m llik_m r_m(b) + beta ((1 - alpha) kl[M][b] + alpha / M sum_e kl[e][b]) ]

    `alpha` in [0, 1] comes from the config's `model_cfg: {alpha: ...}` (default 5/6).  The experts enter the KL terms
    with the numbers the product gave them (variance used as the scale, the convention of every mixer here).  The latent
    side of a step is ONE fused kernel each way (ops.tc_fusion).  Inference, the evaluation hooks and the metrics are POE's
    on the product without the prior expert."""

    prior_expert = False

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        self._refuse_beyond_single_pass("mvtcae", vaes, obj_config, "the KL terms between the joint and the experts",
                                        "total-correlation objective", "total-correlation", "step")
        alpha = float((model_config or {}).get("alpha", 5.0 / 6.0))
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"mvtcae: model_cfg alpha = {alpha} must lie in [0, 1]")
        super().__init__(vaes, n_latents, obj_config, model_config)
        self.modelName = "mvtcae"
        self.alpha = alpha

    def _tc_weights(self):
        """rows of the loss assembly (loss, kld, kld_prior, kld_cond) over [M recon rows, M expert KL rows, the prior's]"""
        M, a, beta = len(self.vaes), self.alpha, float(self.obj_fn.beta)
        lam = [float(v.llik_scaling) * (M - a) / M for v in self.vaes.values()]
        return [lam + [beta * a / M] * M + [beta * (1.0 - a)],
                [0.0] * M + [a / M] * M + [1.0 - a],
                [0.0] * M + [0.0] * M + [1.0],
                [0.0] * M + [1.0 / M] * M + [0.0]]

    def objective(self, mods):
        """one encoder pass and one decoder pass per modality (POE: 2^(M-1) and 2^M - 1), the towers on their streams"""
        def fuse(theta, packed, B, D, dev, raw):
            _, kl, z = ops.tc_fusion(theta, packed, self._draw(B, D, dev), theta.grad, raw=raw)
            return z, kl, {}
        return self._single_pass_objective(mods, fuse, ("kld_prior", "kld_cond"), self._tc_weights())


class MOE(TorchMMVAE):
    """MMVAE, mixture of experts (mmvae_models.py:10-131): objective "elbo" with K = 1, "dreg"
    with any K on towers that keep the K axis (the shipped configs/config_mnistsvhn.yml: MNIST / SVHN towers, K = 30,
    `prior: laplace`) and "iwae" with any K on any towers (literal where the reference runs -- B = 1 or K = 1 --, a
    defined extension with the K-preserving text decoder beyond: MultimodalObjective.iwae; BASELINE configs[2] =
    iwae, K = 8, CdSprites+ towers).  elbo with K > 1 fails in the reference.

    q_m = Normal | Laplace(mu_m, scale = lv_m) -- the config's `prior` key also names the posterior and the likelihood
    family (models/trainer.py:104) --, K samples z_m per modality; every modality is decoded from its own z
    (likelihood Normal, :101-103) and from the z of the LAST other modality (likelihood `vae.px_z`, the dict overwrite
    of :112-116).
    elbo: KL against the per-VAE fixed N(0,1) prior through the model-level `self.pz` = Normal (:45); cross terms
      weighted by exp(log q_r(z_o) - log q_o(z_o).detach()) with z_o detached; rows whose weighted sum is exactly 0
      are dropped and beta*kld.sum() is subtracted once per surviving row (:73, objectives.py:67); loss / M.
    dreg: objectives.py:361-387 with the TRAINABLE model prior N(0, softmax(theta) D) (:76, pz_params)."""

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        super().__init__(vaes, n_latents, **obj_config)
        self.model_config = model_config
        self.modelName = "moe"
        obj = self.obj_fn.obj_name
        if obj == "elbo" and self.K != 1:
            raise NotImplementedError("moe: obj elbo with K > 1 fails in the reference (mmvae_models.py:62); use dreg")
        if obj in ("dreg", "iwae") and len(self.vaes) != 2:
            raise NotImplementedError("moe dreg / iwae: the reference's cross-term indexing (mmvae_models.py:64-70) is "
                                      "only meaningful for two modalities")
        for vae in self.vaes.values():
            if vae.prior_str not in ("normal", "gaussian", "laplace"):
                raise NotImplementedError(f"prior: {vae.prior_str} is not on the MI355X path (normal, laplace are)")
        self._laplace = [v.prior_str == "laplace" for v in self.vaes.values()]
        self.register_buffer("_theta0", torch.zeros(1, n_latents), persistent=False)   # softmax(0)*D = 1: N(0,1)

    batch_passes = True      # elbo: a decoder's own + cross pass in one call (objective)

    def _draw_k(self, m, K, B, D, dev):
        """(K,B,D) standard variates of q_m's family: one recorded draw (`eps_override`) or the device generator"""
        if self.eps_override is not None:
            return self.eps_override.pop(0).reshape(K, B, D).to(device=dev, dtype=torch.float32).contiguous()
        return (ops.rand_laplace if self._laplace[m] else ops.randn)((K, B, D), self._rng_state)

    def objective(self, data):
        """mmvae_models.py:32-78"""
        if self.obj_fn.obj_name in ("dreg", "iwae"):        # same forward; the objective differs (objectives.py)
            return self._objective_dreg(data)
        self._begin_step()
        names = list(self.vaes.keys())
        M = len(names)
        # Round 4: the towers on two streams (encoders side by side, decoders + their loss terms side by side; autograd
        # replays every node on its forward stream), and each decoder's own + cross pass as ONE call over 2 B latent
        # samples (rows [0, B) decode z_r, rows [B, 2B) z_o; the row-sum kernels pair output row k with target row k % B).
        # Same sums; a decoder with dropout draws its masks once for both passes (independent masks either way: the
        # extracted-mask parity test splits them by pass).  optimal_sigma fits ONE sigma per call: its passes stay apart.
        # The shipped config_cdspritesplus.yml step is a chain of ~260 launches, ~115 of them the text decoder's two
        # op-by-op passes: 4.00 -> 3.4 ms/step.
        packed, streams, dev, _ = self._encode_towers(data)
        B, D = packed[0].shape[0], self.n_latents
        zs, kls = [], []
        for i in range(M):
            eps = self._draw_k(i, 1, B, D, dev).reshape(B, D)
            if self._laplace[i]:      # z = mu + scale * e all the same; KL(Laplace || N(0,1)) has its own closed form
                _, _, z = ops.poe_reparam_kl(self._theta0, [packed[i]], [eps], 2, 0)
                kls.append(ops.kl_laplace_normal(packed[i]))
            else:
                _, kl, z = ops.poe_reparam_kl(self._theta0, [packed[i]], [eps], 2, 0b10)
                kls.append(ops.kl_row(kl, 1))      # (kl_mask 0b10: row 1 is the only one the backward reads)
            zs.append(z[0])
        def decode(r, st):
            vae = self.vaes[names[r]]
            mod = data[names[r]]
            o = [s for s in range(M) if s != r][-1]
            mk = mod["masks"]
            if vae.ltype != "optimal_sigma" and self.batch_passes:
                z2 = torch.cat([zs[r], zs[o]], 0)
                out, _ = vae.dec({"latents": z2.unsqueeze(0), "masks": None if mk is None else mk.repeat(2, 1)})
                # own: dist.Normal(*px_z) (:101-103); cross (rows B..2B): vae.px_z = the config's `prior` family (:115)
                rs = recon_rowsum(vae.ltype, out, mod, laplace=(0b10, B) if self._laplace[r] else False)
                own_r, cross_r = rs.view(2, B).unbind(0)      # (backward: one stack instead of two zero-fill + copy pairs)
            else:
                own, _ = vae.dec({"latents": zs[r].unsqueeze(0), "masks": mk})
                cross, _ = vae.dec({"latents": zs[o].unsqueeze(0), "masks": mk})
                own_r = recon_rowsum(vae.ltype, own, mod)
                cross_r = recon_rowsum(vae.ltype, cross, mod, laplace=self._laplace[r])
            ratio = ops.laplace_logratio if self._laplace[r] else ops.normal_logratio
            lw = ratio(packed[r], packed[o].detach(), zs[o].detach())
            return own_r, ops.expmul(lw, cross_r)
        # (the heads and the samples are read by both towers' decoder sides)
        rows = [t for pair in self._tower_phase(enumerate(streams), decode, dev, reads=packed + zs, batch=data) for t in pair]
        W = [float(vae.llik_scaling) for vae in self.vaes.values() for _ in range(2)]
        kld = torch.stack(kls)                                              # (M, B), also the logged "kld"
        loss = ops.moe_elbo(rows, W, kld, self.obj_fn.beta, M)
        with torch.no_grad():                                               # logged only: lpx rows, reference sign
            lpx = list(torch._foreach_mul([r.detach() for r in rows], [-w for w in W]))      # (one launch)
        return {"loss": loss, "reconstruction_loss": lpx, "kld": kld}

    def _objective_dreg(self, data):
        """MOE.objective's non-elbo branch + MultimodalObjective.dreg / .iwae (mmvae_models.py:63-78,
        objectives.py:342-387).  Every decoder decodes ALL M*K*B latent samples in one pass (rows [r*K*B, (r+1)*K*B) are
        z_r): its own block is the own reconstruction, the other block the cross reconstruction.  dreg: `lprob` towers
        that keep K (its lw sums over the batch per k, which only those towers' (K,) sums allow); iwae: any tower, the
        target rows repeat over (r, k) inside the loss kernels (row % B)."""
        self._begin_step()
        names = list(self.vaes.keys())
        M, K, D = len(names), int(self.K), self.n_latents
        packed, streams, dev, _ = self._encode_towers(data)
        B = packed[0].shape[0]
        eps = [self._draw_k(m, K, B, D, dev) for m in range(M)]
        theta = self._pz_params[1]
        iwae = self.obj_fn.obj_name == "iwae"
        # lat = log p(z) - beta lqz: dreg has no beta (objectives.py:372), iwae multiplies lqz by it (:356)
        lat, z = ops.moe_ksample(theta, packed, eps, self._laplace, theta.grad,
                                 beta=float(self.obj_fn.beta) if iwae else 1.0)          # z: (M,K,B,D)
        KB = K * B
        def decode(r, st):
            n = names[r]
            vae = self.vaes[n]
            if not iwae and (vae.ltype != "lprob" or data[n]["masks"] is not None):
                raise NotImplementedError("moe dreg: recon_loss lprob on unmasked modalities (the MNIST / SVHN towers) "
                                          "is what keeps the K axis in the reference")
            self.obj_fn.set_ltype(vae.ltype)
            o = 1 - r
            out, _ = vae.dec({"latents": z.view(M * K, B, D), "masks": data[n]["masks"]})     # (M*K, B, ...) / (M*K*B, ...)
            # own block r: dist.Normal (:101-103); cross block o: vae.px_z = the config's `prior` family (:115)
            lap_mask = (1 << o) if self._laplace[r] else 0
            if vae.ltype == "optimal_sigma":
                # optimal_sigma fits ONE sigma per reference call, and the reference evaluates the own and the cross
                # reconstruction in separate calls (mmvae_models.py:63-78): row sums per source posterior (found by
                # the K-sample test on the action towers, round 5: one sigma over all M K B rows was 9e-4 off)
                flat = out.reshape(M, KB, *out.shape[-3:]) if out.dim() >= 4 else out.reshape(M, KB, -1)
                blocks = [recon_rowsum(vae.ltype, flat[m], data[n]) for m in range(M)]
            else:
                rs = recon_rowsum(vae.ltype, out, data[n], laplace=(lap_mask, KB))          # (M*K*B,)
                blocks = rs.view(M, KB).unbind(0)
            return blocks[r], blocks[o]
        rows = [t for pair in self._tower_phase(enumerate(streams), decode, dev, reads=[z], batch=data) for t in pair]
        lam = [float(vae.llik_scaling) for vae in self.vaes.values()]
        return self.obj_fn.calculate_loss({"lat": lat, "rows": rows, "lam": lam})

    def modality_mixing(self, mods):
        return self.encode(mods)

    def _proposal_size(self, n_given):
        return n_given

    def _proposal(self, mods, given):
        """the unimodal posteriors of `given`: (mu, "logvar" used as scale), Normal | Laplace per modality"""
        names = list(self.vaes.keys())
        comps = torch.stack([packed_head(*self.vaes[m].enc(mods[m])) for m in given])
        return comps, [self._laplace[names.index(m)] for m in given]

    def _sample(self, x, K=1, of=None):
        """K draws per present modality from its own posterior, in modality order; a missing modality takes the latent
        sample of the FIRST present one (the reference aliases that modality's dict, mmvae_models.py:105-108)"""
        _, filled = self.get_missing_modalities(x)
        assert len(filled) > 0, "at least one modality must be present for forward call"
        src = {m: (m if m in filled else filled[0]) for m in self.vaes}
        qz, drawn = {}, {}
        for m, vae in self.vaes.items():
            data = x[m]["data"]
            if data is None:
                qz[m] = None
            elif of is not None and m != src[of]:
                # (latents_for: a present modality nobody samples from has its draw taken, its encoder is not run)
                self._draws(K, data.shape[0], self.n_latents, data.device)
            else:
                mu, lv = vae.enc(x[m])
                qz[m] = normal(mu, lv)
                drawn[m] = mu + lv * self._draws(K, *mu.shape, mu.device)
        return qz, [(m, drawn[src[m]]) for m in self.vaes if src[m] in drawn]

    def _unimodal(self, head):
        """(the reference builds these posteriors with the VAE's own `qz_x`: Laplace under `prior: laplace`)"""
        names = list(self.vaes.keys())
        return {m: (q.loc, q.scale, dist.Laplace if self._laplace[names.index(m)] else dist.Normal)
                for m, q in head.items() if q is not None}

    def forward(self, x, K=1):
        """mmvae_models.py:80-117, including the cross-generation calls with missing modalities
        (`data` None, masks kept: models/trainer.py:179-215): a missing modality is decoded from the sample it borrowed
        under its own masks; every target's cross entry is a fresh one-entry dict, so the last source in dict order wins
        (:109-114)."""
        qz, zs = self._sample(x, K)
        zs = {m: {"latents": z, "masks": x[m]["masks"]} for m, z in zs}      # modality order, as the reference's dict
        px, cross = {}, {}
        for m, vae in self.vaes.items():
            px[m] = normal(*vae.dec({"latents": zs[m]["latents"], "masks": x[m]["masks"]}))
        for src, z in zs.items():
            for tgt, vae in self.vaes.items():
                if tgt != src:
                    cross[tgt] = {src: normal(*vae.dec({"latents": z["latents"], "masks": x[tgt]["masks"]}))}
        return self.make_output_dict(qz, px, zs, cross_decoder_dist=cross)


class MMJSD(MOE):
    """mmJSD, Jensen-Shannon objective (Sutter, Daunhawer, Vogt, NeurIPS 2020; not in the reference: a plugin on the base
    class's contract).  The unimodal posteriors are MOE's, q_e = N(mu_e, sigma = lv_e); the KL of the mixture to the prior
    is replaced by the Jensen-Shannon divergence of the M posteriors and the prior N(0, softmax(theta) D) with weights pi:
    every one's KL to their weighted geometric mean, the dynamic prior.  Row b draws its latent from ONE expert,
    sel[b] = (b M) // B (contiguous balanced chunks, the paper's mixture-component selection), and every modality is
    decoded once from it (MOE's elbo: twice).  With r_m the reconstruction row sums (the sign POE gives them), kl[e] the
    experts' rows and kl[M] the prior's:

        loss = sum_b [ sum_m llik_m r_m(b) + beta (sum_e pi_e kl[e][b] + pi_M kl[M][b]) ]

    `model_cfg: {prior_weight: w}`, 0 < w < 1, gives pi_M = w and every expert (1 - w) / M; the default is the paper's
    uniform 1 / (M + 1).  The latent side of a step is ONE fused kernel each way (ops.js_fusion).  Inference, the
    evaluation hooks and the metrics are MOE's, unchanged: conditioning on several modalities is the MIXTURE over their
    posteriors, the dynamic prior is a training-time regulariser only."""

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        self._refuse_beyond_single_pass("mmjsd", vaes, obj_config, "the geometric mean and the KL terms to it",
                                        "Jensen-Shannon objective", "Jensen-Shannon", "step")
        M = len(vaes)
        w = float((model_config or {}).get("prior_weight", 1.0 / (M + 1)))
        if not 0.0 < w < 1.0:
            raise ValueError(f"mmjsd: model_cfg prior_weight = {w} must lie in (0, 1)")
        super().__init__(vaes, n_latents, obj_config, model_config)
        self.modelName = "mmjsd"
        self.prior_weight = w
        self._sel = {}      # (B, M, device) -> the rows' expert indices, built once: the captured step only reads it

    def _js_pi(self):
        """pi_0 .. pi_M: the experts' weights and, last, the prior's"""
        M = len(self.vaes)
        return [(1.0 - self.prior_weight) / M] * M + [self.prior_weight]

    def _js_weights(self):
        """rows of the loss assembly (loss, kld, kld_prior, kld_experts) over [M recon rows, M expert KL rows, the prior's]"""
        M, beta, pi = len(self.vaes), float(self.obj_fn.beta), self._js_pi()
        lam = [float(v.llik_scaling) for v in self.vaes.values()]
        return [lam + [beta * p for p in pi],
                [0.0] * M + pi,
                [0.0] * M + [0.0] * M + [1.0],
                [0.0] * M + [1.0 / M] * M + [0.0]]

    def _selection(self, B, dev):
        """sel[b] = (b M) // B as int32 on the device"""
        M = len(self.vaes)
        key = (B, M, str(dev))
        if key not in self._sel:
            self._sel[key] = ((torch.arange(B, dtype=torch.int64) * M) // B).to(device=dev, dtype=torch.int32)
        return self._sel[key]

    def objective(self, mods):
        """one encoder pass and one decoder pass per modality (MOE's elbo: one and two), the towers on their streams"""
        def fuse(theta, packed, B, D, dev, raw):
            _, kl, z = ops.js_fusion(theta, packed, self._draw(B, D, dev), self._selection(B, dev), self._js_pi(), theta.grad,
                                     raw=raw)
            return z, kl, {}
        return self._single_pass_objective(mods, fuse, ("kld_prior", "kld_experts"), self._js_weights())


class MMVM(MOE):
    """MMVM VAE, mixture-of-experts prior (Sutter et al., "Unity by Diversity", NeurIPS 2024; not in the reference: a plugin
    on the base class's contract).  Nothing is aggregated: every modality keeps its own posterior q_m = N(mu_m, sigma = lv_m)
    (MOE's), its own sample z_m and decodes itself from it alone.  The fixed prior is replaced by a data-dependent one,
    h = (1/M) sum_j q_j of the same sample, which pulls the M posteriors towards each other.  With r_m the reconstruction
    row sums (the sign POE gives them), kl_mix[m] = log q_m(z_m) - log h(z_m), the one-sample estimate of KL(q_m || h), and
    kl_std[m] = KL(q_m || N(0, softmax(theta) D)) in closed form:

        loss = sum_b [ sum_m llik_m r_m(b) + beta sum_m (alpha kl_mix[m][b] + (1 - alpha) kl_std[m][b]) ]

    `model_cfg: {alpha: a}`, 0 <= a <= 1, default 1 (the paper's objective); a = 0 is M independent VAEs, at a = 1 the
    prior parameter receives an exactly zero gradient.  The latent side of a step is ONE fused kernel each way
    (ops.mixprior_fusion).  Inference, the evaluation hooks and the metrics are MOE's, unchanged.  With the default alpha
    the objective matches nothing to N(0, 1): joint generation should draw from a density fitted to the latents
    (fit_latent_density / sample_latent_density, handed to the metrics as eps= / joint_eps=)."""

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        self._refuse_beyond_single_pass("mmvm", vaes, obj_config, "the mixture prior's densities and the KL terms",
                                        "mixture-of-experts prior", "mixture-prior", "modality and step")
        alpha = float((model_config or {}).get("alpha", 1.0))
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"mmvm: model_cfg alpha = {alpha} must lie in [0, 1]")
        super().__init__(vaes, n_latents, obj_config, model_config)
        self.modelName = "mmvm"
        self.alpha = alpha

    def _mm_weights(self):
        """rows of the loss assembly (loss, kld, kld_mix, kld_std) over [M recon rows, M kl_mix rows, M kl_std rows]"""
        M, a, beta = len(self.vaes), self.alpha, float(self.obj_fn.beta)
        lam = [float(v.llik_scaling) for v in self.vaes.values()]
        return [lam + [beta * a] * M + [beta * (1.0 - a)] * M,
                [0.0] * M + [a] * M + [1.0 - a] * M,
                [0.0] * M + [1.0] * M + [0.0] * M,
                [0.0] * M + [0.0] * M + [1.0] * M]

    def objective(self, mods):
        """one encoder pass and one decoder pass per modality (MOE's elbo: one and two), the towers on their streams"""
        def fuse(theta, packed, B, D, dev, raw):
            M = len(packed)
            if self.eps_override is not None:      # M recorded draws, in modality order
                eps = torch.stack([self._draw(B, D, dev) for _ in range(M)])
            else:
                eps = ops.randn((M, B, D), self._noise_state())
            zs, kl, resp = ops.mixprior_fusion(theta, packed, eps, theta.grad, raw=raw)
            # 1 / M: the posteriors are indistinguishable; 1: they are disjoint and the regulariser's gradient has vanished
            return zs, kl, {"resp_self": lambda: resp.diagonal(dim1=0, dim2=1).mean()}
        return self._single_pass_objective(mods, fuse, ("kld_mix", "kld_std"), self._mm_weights())


class DMVAE(TorchMMVAE):
    """DMVAE, shared + private latents (mmvae_models.py:413-509), K = 1, all modalities present.

    Every encoder emits D + P columns; [:D] is the shared posterior, [D:] the private one (split after the softmax
    over all D + P columns, mmvae_base.py:152-156).  joint = product of the shared experts, no prior expert.  Noise is
    drawn in the reference's order: z_joint, then per modality z_shared, z_private and a fresh shared draw of every
    other modality for the cross reconstruction.  Three ELBOs per modality (:458-459), all summed over the batch."""

    def __init__(self, vaes, n_latents: int, obj_config: dict, model_config=None):
        super().__init__(vaes, n_latents, **obj_config)
        self.model_config = model_config
        self.modelName = "dmvae"
        self._require_normal_priors()
        assert self.latent_factorization, "DMVAE requires private_latents in the config"
        if self.K != 1:
            raise NotImplementedError("dmvae: K = 1 only on this path")
        pmax = max(v.private_latents for v in self.vaes.values())
        self.register_buffer("_theta0", torch.zeros(1, pmax), persistent=False)    # N(0,1) prior of the private part

    batch_passes = True      # a decoder's own + joint + cross passes in one call (objective)

    def objective(self, mods):
        self._begin_step()
        names = list(self.vaes.keys())
        M, D = len(names), self.n_latents
        beta = float(self.obj_fn.beta)
        theta = self._pz_params[1]
        # Round 4: towers on two streams (as MOE.objective), and a decoder's passes -- own, joint, cross (one per other
        # modality) -- as ONE call over (2 + (M - 1)) B latent samples (the row-sum kernels pair output row k with target
        # row k % B; a decoder with dropout draws its masks once for all passes; optimal_sigma fits one sigma per call:
        # its passes stay apart).  BASELINE configs[3]: 1.54 -> 1.2 ms/step.
        packed, streams, dev, _ = self._encode_towers(mods)
        B = packed[0].shape[0]
        P = [self.vaes[n].private_latents for n in names]
        # noise in the reference's draw order (mmvae_models.py:486-502)
        e_sh, e_pr, e_cross = {}, {}, {}
        if self.eps_override is None and len(set(P)) == 1:
            # two launches instead of 1 + M (M + 1): every D-wide draw of the step from one (n, B, D) block, the private
            # ones from one (M, B, P) block (independent standard normals either way; recorded noise keeps the order below)
            wide = self._draw_many(1 + M * M, B, D, dev)
            priv = self._draw_many(M, B, P[0], dev)
            e_joint, k = wide[0], 1
            for i in range(M):
                e_sh[i], e_pr[i], k = wide[k], priv[i], k + 1
                for m in range(M):
                    if m != i:
                        e_cross[(i, m)], k = wide[k], k + 1
        else:
            e_joint = self._draw(B, D, dev)
            for i in range(M):
                e_sh[i] = self._draw(B, D, dev)
                e_pr[i] = self._draw(B, P[i], dev)
                for m in range(M):
                    if m != i:
                        e_cross[(i, m)] = self._draw(B, D, dev)        # target i, fresh draw of q_shared(m)
        _, klj, zj = ops.poe_reparam_kl(theta, packed, [e_joint], 0, 1 << M, theta.grad, cols=(0, D))
        z_sh, z_cr, kl_sh, z_pr, kl_pr = {}, {}, {}, {}, {}
        for m in range(M):
            targets = [i for i in range(M) if i != m]
            _, kl, z = ops.poe_reparam_kl(theta, [packed[m]], [e_sh[m]] + [e_cross[(i, m)] for i in targets], 2, 0b10,
                                          theta.grad, cols=(0, D))
            z_sh[m], kl_sh[m] = z[0], kl                    # (kl: (2, B), the posterior's KL is row 1)
            for i, zc in zip(targets, z[1:]):
                z_cr[(i, m)] = zc
            _, klp, zp = ops.poe_reparam_kl(self._theta0[:, :P[m]].contiguous(), [packed[m]], [e_pr[m]], 2, 0b10, None,
                                            cols=(D, P[m]))
            z_pr[m], kl_pr[m] = zp[0], klp
        # every decoder's input batch -- rows [own | joint | cross...] x columns [shared | private] -- from ONE launch for all
        # modalities, and every sample's gradient as one sum in backward (ops.RowsFan): 2 cat + 1 repeat per modality forward,
        # a repeat-sum, the strided slices' copies and an addition per shared sample backward before
        batched = [self.vaes[n].ltype != "optimal_sigma" and self.batch_passes for n in names]
        lats = None
        if all(batched) and zj[0].is_cuda:
            srcs, index, plan = [], {}, []

            def src(t):
                if id(t) not in index:
                    index[id(t)] = len(srcs)
                    srcs.append(t)
                return index[id(t)]
            for i in range(M):
                zs_i = [z_sh[i], zj[0]] + [z_cr[(i, m)] for m in range(M) if m != i]
                plan.append((len(zs_i), D + P[i], [(src(z), k, 0) for k, z in enumerate(zs_i)] +
                             [(src(z_pr[i]), k, D) for k in range(len(zs_i))]))
            if ops.RowsFan.supported(plan, srcs):
                lats = ops.rows_fan(plan, srcs)

        def decode(i, st):
            n = names[i]
            vae = self.vaes[n]
            zs_i = [z_sh[i], zj[0]] + [z_cr[(i, m)] for m in range(M) if m != i]      # decode order own, joint, cross
            mk = mods[n]["masks"]                                                  # (mmvae_models.py:494-502)
            if vae.ltype != "optimal_sigma" and self.batch_passes:
                NP = len(zs_i)
                lat = lats[i] if lats is not None else torch.cat([torch.cat(zs_i, 0), z_pr[i].repeat(NP, 1)], -1)
                out, _ = vae.dec({"latents": lat.unsqueeze(0), "masks": None if mk is None else mk.repeat(NP, 1)})
                rs = recon_rowsum(vae.ltype, out, mods[n], laplace=self._lap(vae))
                return [rs.view(NP, B)]                    # ONE (passes, B) block: rows own, joint, cross...
            blocks = []
            for z in zs_i:
                out, _ = vae.dec({"latents": torch.cat([z, z_pr[i]], -1).unsqueeze(0), "masks": mk})
                blocks.append(recon_rowsum(vae.ltype, out, mods[n], laplace=self._lap(vae)).view(1, B))
            return blocks
        reads = [zj[0]] + list(z_sh.values()) + list(z_cr.values()) + list(z_pr.values()) + list(lats or [])
        per = self._tower_phase(enumerate(streams), decode, dev, reads=reads, batch=mods)
        # ELBO assembly on the calls' row BLOCKS (as POE.objective: selecting rows out of the batched row sums / the KL
        # blocks cost a zero-fill and a copy per row in autograd's select / unbind backward -- 15 launches per step at
        # M = 2): every block is addressed in place, a row that does not enter an output has weight 0
        blocks, W_loss, W_kld = [], [], []
        W_ind = [[] for _ in range(M)]

        def put(blk, wl, wk, ind_of=None):
            blocks.append(blk)
            W_loss.extend(wl)
            W_kld.extend(wk)
            for j in range(M):
                W_ind[j].extend([1.0 if (j == ind_of and r == 0) else 0.0 for r in range(len(wl))])
        for i, n in enumerate(names):
            lam = float(self.vaes[n].llik_scaling)
            first = True
            for blk in per[i]:                                  # rows in decode order: own, joint, cross...
                r = blk.shape[0]
                put(blk, [lam] * r, [0.0] * r, i if first else None)
                first = False
            put(kl_sh[i], [0.0, beta], [0.0, 1.0 / M])
            put(kl_pr[i], [0.0, beta * (M - 1)], [0.0, 0.0])
        put(klj, [0.0] * M + [beta * M], [0.0] * (M + 1))       # the joint's KL (last row) enters every modality's joint ELBO
        if len(W_loss) <= 32 and M <= 2:
            out = ops.lincomb_rows(blocks, [W_loss, W_kld] + W_ind)
            ind = [o.detach() for o in out[2:]]
        elif len(W_loss) <= 32:
            out = ops.lincomb_rows(blocks, [W_loss, W_kld])
            ind = [per[i][0][0].detach().sum() for i in range(M)]
        else:       # (more rows than one assembly launch addresses: the selected rows only)
            rows, W_loss, W_kld = [], [], []
            for i, n in enumerate(names):
                lam = float(self.vaes[n].llik_scaling)
                flat_rows = [r_ for blk in per[i] for r_ in blk.unbind(0)]
                own, joint, cross = flat_rows[0], flat_rows[1], flat_rows[2:]
                rows += [own, kl_sh[i][1], joint, klj[M]] + cross + [kl_pr[i][1]]
                W_loss += [lam, beta, lam, beta] + [lam] * len(cross) + [beta * len(cross)]
                W_kld += [0.0, 1.0 / M, 0.0, 0.0] + [0.0] * len(cross) + [0.0]
            out = ops.lincomb_rows(rows, [W_loss, W_kld])
            ind = [per[i][0][0].detach().sum() for i in range(M)]
        return {"loss": out[0], "reconstruction_loss": ind, "kld": out[1]}

    def modality_mixing(self, mods):
        return self.encode(mods)

    def _sample(self, x, K=1, of=None):
        """mmvae_models.py:467-503, missing modalities (`data` None, masks kept) included: the joint is the product of
        the PRESENT shared experts; a missing modality samples its shared code from the first present modality's
        posterior and its private code from N(0, I) (:489-493); cross reconstructions from a fresh shared draw of every
        other present modality (:499-502).  Draws in the reference's order: z_joint, then per modality z_shared,
        z_private and, as they are read, one (source, z) per other present modality.
        -> ((posteriors of encode(), joint (mu, variance), z_joint), (modality, z_shared, z_private, cross draws))"""
        if K != 1:
            raise NotImplementedError("dmvae.forward: K = 1 only on this path")
        _, filled = self.get_missing_modalities(x)
        assert len(filled) > 0, "at least one modality must be present for forward call"
        D, first = self.n_latents, x[filled[0]]["data"]
        src = {n: (n if n in filled else filled[0]) for n in self.vaes}
        if of is None:
            enc_d = self.encode(x)
            joint = self.product_of_experts([enc_d[n]["shared"][0] for n in filled],
                                            [enc_d[n]["shared"][1] for n in filled])
        else:      # (latents_for: only the tower `of` samples from is run, the joint's draw is taken without its product)
            enc_d, joint = self.encode(self._given_only(x, [src[of]])), None

        def draw(post, d):      # a posterior that was not encoded (or does not exist: a missing private code) gives N(0, I)
            e = self._draw(first.shape[0], d, first.device).unsqueeze(0)
            return e if post is None else post[0] + post[1] * e

        def per_modality():
            for n, vae in self.vaes.items():
                z_shared = draw(enc_d[src[n]]["shared"], D)
                if n == of:      # (latents_for stops here: the evaluation generator moves no further than this draw)
                    yield n, z_shared
                    return
                z_private = draw(enc_d[n]["private"], vae.private_latents)
                cross = ((m, draw(enc_d[m]["shared"], D)) for m in filled if m != n)
                yield n, z_shared, z_private, cross
                for _ in cross:      # (latents_for: the cross draws nobody decoded are taken all the same)
                    pass
        return (enc_d, joint, draw(joint, D)), per_modality()

    def _unimodal(self, head):
        return {m: (*q["shared"], dist.Normal) for m, q in head[0].items() if q["shared"] is not None}

    def _joint_posterior(self, head):
        """the product of the shared experts (mu, variance used as scale): the shared code's joint"""
        return None if head[1] is None else (head[1][0], head[1][1])

    def forward(self, x, K=1):
        """mmvae_models.py:467-503: the container the evaluation code reads (shared / private posteriors, joint
        posterior, own / joint / cross reconstructions); every reconstruction is decoded right behind its draw."""
        (enc_d, joint, z_joint), zs = self._sample(x, K)
        joint_d = normal(*joint)
        joint_dist, qz_xs, qz_private, zss, px_zs, joint_px_zs, cross_px_zs = {}, {}, {}, {}, {}, {}, {}
        for n, z_shared, z_private, cross in zs:
            vae, masks = self.vaes[n], x[n]["masks"]
            joint_dist[n] = joint_d
            qz_xs[n] = normal(*enc_d[n]["shared"]) if enc_d[n]["shared"] is not None else None
            qz_private[n] = normal(*enc_d[n]["private"]) if enc_d[n]["private"] is not None else None
            dec = lambda z: self._px(vae, *vae.dec({"latents": torch.cat([z, z_private], -1), "masks": masks}))
            zss[n] = {"latents": z_shared, "masks": masks}
            px_zs[n] = dec(z_shared)
            joint_px_zs[n] = dec(z_joint)
            cross_px_zs[n] = {m: dec(z) for m, z in cross}
        return self.make_output_dict(qz_xs, px_zs, zss, joint_dist, qz_private, None, joint_px_zs, cross_px_zs)
