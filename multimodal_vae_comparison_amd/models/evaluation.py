"""The evaluation metrics of TorchMMVAE (DESIGN.md sections 7a-7o) as a mixin: held-out log-likelihood, latent
classification, CdSprites+ and MNIST-SVHN generation coherence, latent analysis, Frechet distance, precision / recall /
density / coverage and kernel inception distance of generated images, the disentanglement of the latent code, the
cross-modal (canonical) correlation of generations, the cluster analysis of the latents and the reconstruction quality of
generated images against the images they were generated for (PSNR, SSIM, MS-SSIM) and of generated text against the captions
it was generated for (error rates, BLEU, ROUGE-L, perplexity), the cross-modal retrieval of latents (recall@k, median
rank, MRR), and the ex-post density estimation of the latents (a Gaussian mixture per conditioning subset, and draws from it
for the joint metrics), and the kernel two-sample tests of the latents against the prior, each other and a fitted density
(MMD^2 with a permutation null), and the sliced Wasserstein distances and per-dimension Kolmogorov-Smirnov tests of the
same latent sets and of generated against real rows.  What they share is here once: the
guard (`_need_eval`), the noise context (`_eval_noise`), the joint metrics' prior sample (`_prior_sample`), the modality
lookup (`_find_modalities`), the walk over real and generated feature sets (`_walk_generations`).  The mixers override the
hooks `_proposal_size`, `_proposal`, `_sample`, `_unimodal` and `_joint_posterior`."""
import contextlib
import itertools

import numpy as np
import torch
import torch.distributions as dist

from .. import coherence as coh, ops
from .decoders import Dec_TxtTransformer
from .objectives import recon_rowsum

# what dropout would make of a metric: the reason clauses of `_need_eval`
_LATENTS = "the latents a function of the masks"
_GENERATIONS = "the generations a function of the masks"


class EvaluationMixin:
    def _need_eval(self, who, why, shared_latents=False):
        """the guard of metric `who`: eval mode (`why`: what dropout would make of the result) and, `shared_latents`,
        one latent space -- the joint metrics decode a prior sample, which models with private latents (DMVAE) lack"""
        if self.training:
            raise RuntimeError(f"{who} needs eval mode (model.eval()): dropout would make {why}")
        if shared_latents and self.latent_factorization:
            raise NotImplementedError(f"{self.modelName}: {who} is built for the mixers with one shared latent space "
                                      f"(poe, moe, mopoe); private latents have no joint prior sample")

    @contextlib.contextmanager
    def _eval_noise(self, eps=None, keep_override=False):
        """Inside: no gradients, and forward()'s draws come from the evaluation generator (`_noise_state`): the training
        noise state stays as it is.  `eps_override` is None for the duration (the generator draws) or a fresh list copy of
        `eps`, consumed in forward()'s draw order; what the model held comes back afterwards.  `keep_override`
        (latents_for) leaves `eps_override` alone: recorded draws of the caller's are consumed as forward() consumes them."""
        saved, was = self.eps_override, self._eval_draws
        if not keep_override:
            self.eps_override = None if eps is None else [e for e in eps]
        self._eval_draws = True
        try:
            with torch.no_grad():
                yield
        finally:
            self._eval_draws = was
            if not keep_override:
                self.eps_override = saved

    def _prior_sample(self, n, eps, who):
        """(1, n, D): n latents z ~ p(z) = Normal(*pz_params), as the decoders take them.  The draw comes from the
        evaluation generator, or is `eps` (n, D).  (Private latents are the guard's to refuse: before the caller checks
        its classifiers, `n` after.)"""
        n = int(n)
        if n < 1:
            raise ValueError(f"{who}: n = {n}")
        (loc, scale), D = self.pz_params, self.n_latents
        e = (ops.randn((n, D), self._noise_state(evaluation=True)) if eps is None
             else eps.to(device=loc.device, dtype=torch.float32).reshape(n, D))
        return (loc + scale * e).unsqueeze(0).contiguous()

    def _find_modalities(self, who, wanted, only_two=False):
        """names of the modalities a metric works on.  `wanted`: (argument name, the caller's choice or None,
        predicate on a data_dim tuple) per modality; a None becomes the one modality whose data_dim passes the predicate
        (`only_two`: of a model with exactly two modalities).  The names must exist and differ."""
        names = list(self.vaes.keys())
        out = []
        for what, given, is_it in wanted:
            if given is None:
                hit = [m for m in names if is_it(tuple(self.vaes[m].data_dim))]
                if len(hit) != 1 or (only_two and len(names) != 2):
                    raise ValueError(f"{who}: name the `{what}` modality (this model has {names})")
                given = hit[0]
            out.append(given)
        if any(m not in names for m in out) or len(set(out)) != len(out):
            said = ", ".join(f"{what} = {m!r}" for (what, _, _), m in zip(wanted, out))
            raise ValueError(f"{who}: {said} are not two modalities of this model ({names})")
        return out

    def _given_only(self, mods, given):
        """the batch with the `data` of every modality outside `given` set to None (masks kept), as the cross-generation
        calls of forward() take it"""
        return {m: (mods[m] if m in given else dict(mods[m], data=None)) for m in self.vaes}

    def _walk_generations(self, who, batches, features, n_joint, eps, joint_eps, rows_ok, sink):
        """The walk of the metrics that compare the features of real and of generated rows (`who`: frechet_distances,
        manifold_metrics, kernel_distances).  After the guard and the argument checks (`rows_ok(real rows, n_joint)` raises the metric's own
        refusal; all of it before the first forward()), per modality m of `features` every set goes to `sink(m, key, f)`,
        f (rows, F) the extractor's float features, inside the evaluation noise context:
          "real"        every batch's data, all batches first;
          "recon"       forward() of the full batch;
          ("cross", g)  forward() with only modality g given, for every other modality g;
          "joint"       n_joint > 0: the decoder output of n_joint latents z ~ p(z) (`joint_eps` replaces the draw).
        Per batch forward() runs on the full batch, then once per modality g in modality order; of a generation's rows
        the first B (the batch's) are kept.  -> (the modalities walked, in model order; {m: F})."""
        n_joint = int(n_joint)
        self._need_eval(who, _GENERATIONS, shared_latents=n_joint > 0)
        names, batches = list(self.vaes.keys()), list(batches)
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        if not features or any(m not in names or not callable(f) for m, f in features.items()):
            raise ValueError(f"{who}: `features` maps modalities of this model ({names}) to callables")
        mods = [m for m in names if m in features]
        for batch in batches:
            if any(m not in batch or batch[m]["data"] is None for m in names):
                raise ValueError(f"{who}: every batch must hold every modality (a modality without data)")
        rows_ok(sum(len(b[mods[0]]["data"]) for b in batches), n_joint)
        dims = {}

        def hand(m, key, x, keep=None):
            f = features[m](x)
            if not torch.is_tensor(f) or f.dim() != 2 or not f.is_floating_point():
                raise ValueError(f"{who}: the extractor of {m!r} must return float (rows, F) features")
            if dims.setdefault(m, f.shape[1]) != f.shape[1]:
                raise ValueError(f"{who}: the extractor of {m!r} returned F = {f.shape[1]} after F = {dims[m]}")
            sink(m, key, f if keep is None else f[:keep])

        with self._eval_noise(eps):
            for batch in batches:
                for m in mods:
                    hand(m, "real", batch[m]["data"])
            for batch in batches:
                B = len(batch[mods[0]]["data"])
                out = self.forward(batch)
                for m in mods:
                    hand(m, "recon", out.mods[m].decoder_dist.loc, B)
                for g in names:
                    if any(m != g for m in mods):
                        out = self.forward(self._given_only(batch, [g]))
                        for m in mods:
                            if m != g:
                                hand(m, ("cross", g), out.mods[m].decoder_dist.loc, B)
            if n_joint > 0:
                z = self._prior_sample(n_joint, joint_eps, who)
                for m in mods:
                    hand(m, "joint", self.vaes[m].dec({"latents": z, "masks": None})[0])
        return mods, dims

    # ---- held-out log-likelihood ---------------------------------------------------------------
    def _proposal_size(self, n_given):
        """number of mixture components C of q(z | x_G) for |G| = n_given (mixers with a joint proposal override it)"""
        raise NotImplementedError(f"{self.modelName}: estimate_log_likelihood has no joint proposal for this mixer "
                                  f"(poe, moe and mopoe have one; private latents do not)")

    def _proposal(self, mods, given):
        """-> (comps (C,B,2D) = [loc | scale] of the components of q(z | x_G), C Laplace flags)"""
        raise NotImplementedError(f"{self.modelName}: estimate_log_likelihood has no joint proposal for this mixer")

    @staticmethod
    def default_k_chunk(K, C, B):
        """samples per decoder call: the largest multiple of C that divides K with k_chunk * B <= 1024 rows, at least C
        (decoder batches stay inside the range the training paths run at, memory does not grow with K)"""
        best = C
        for kc in range(C, K + 1, C):
            if K % kc == 0 and kc * B <= 1024:
                best = kc
        return best

    def estimate_log_likelihood(self, mods, K, given=None, targets=None, k_chunk=None, eps=None):
        """K-sample importance-sampled bound on the held-out log-likelihood, comparable across mixers.

        `given` G (default: every modality whose data is not None) conditions the proposal, `targets` T (default: the
        same) are the modalities whose likelihood is estimated.
          proposal  q(z | x_G) = (1/C) sum_c q_c(z), the (loc, scale) pairs this model's forward() / modality_mixing()
                    hand to Normal / Laplace (the variance-used-as-scale quirk included):
                    poe: C = 1, the product of the prior expert and the experts of G;  moe: C = |G|, the unimodal
                    posteriors (Normal | Laplace as `_laplace` says);  mopoe: C = 2^|G| - 1, the subset products;
          prior     p(z) = Normal(pz_params) = (location, softmax(theta) D);
          draws     stratified, K % C == 0: sample k comes from component k % C, z[k,b] = loc_c[b] + scale_c[b] eps[k,b];
          lw0[k,b]  = sum_d log p(z[k,b,d]) - log((1/C) sum_c exp sum_d log q_c(z[k,b,d]));
          ll_m[k,b] = log p(x_m[b] | z[k,b]) = -recon_rowsum(ltype_m, dec_m(z), x_m), without llik_scaling;
          joint     = log-mean-exp_k (lw0 + sum_{m in T} ll_m)          <= log p(x_T)        (G = T: the IWAE bound)
          cond[m]   = log-mean-exp_k ll_m, z ~ q(z | x_G)               (the papers' conditional estimate log p(x_m | x_G))
          ess       = exp(2 lse_k(w) - lse_k(2 w)) of the joint weights (effective sample size: judge K by it).
        Returns {"joint": (B,), "cond": {m: (B,)}, "ess": (B,)}, float64.  Needs eval mode (dropout would make the bound
        meaningless); runs without gradients and leaves the training noise state, dropout counters, gradients and the
        optimiser alone.  `k_chunk` samples are decoded per call (default_k_chunk); `eps` (K,B,D) replaces the
        generator (tests).  An optimal_sigma likelihood fits one sigma per decoded (B-row) sample, as the objectives'
        one-sigma-per-call does, so that the estimate does not depend on k_chunk."""
        self._proposal_size(0)      # (a mixer without a joint proposal says so before the batch is looked at)
        names = list(self.vaes.keys())
        given = [m for m in names if mods[m]["data"] is not None] if given is None else [m for m in names if m in given]
        targets = list(given) if targets is None else [m for m in names if m in targets]
        C = self._proposal_size(len(given))
        self._need_eval("estimate_log_likelihood", "the bound meaningless")
        if not given or not targets or any(mods[m]["data"] is None for m in list(given) + targets):
            raise ValueError("estimate_log_likelihood: `given` and `targets` must name modalities with data")
        K = int(K)
        if K < 1 or K % C != 0:
            raise ValueError(f"estimate_log_likelihood: K = {K} must be a positive multiple of the proposal's {C} "
                             f"components (stratified draws)")
        if len(targets) > ops.H.MOE_MAX_MODS or C > ops.H.MIX_MAX_COMPONENTS:
            raise NotImplementedError(f"estimate_log_likelihood: {len(targets)} targets / {C} components (up to "
                                      f"{ops.H.MOE_MAX_MODS} / {ops.H.MIX_MAX_COMPONENTS} are on the MI355X path)")
        with torch.no_grad():       # (no `_eval_noise`: the sampling kernel is handed the evaluation generator's state)
            comps, lap = self._proposal(mods, given)
            _, B, D2 = comps.shape
            D = D2 // 2
            kc = self.default_k_chunk(K, C, B) if k_chunk is None else int(k_chunk)
            if kc < 1 or kc % C != 0 or K % kc != 0:
                raise ValueError(f"estimate_log_likelihood: k_chunk = {kc} must be a multiple of {C} that divides K = {K}")
            if eps is not None:
                eps = eps.to(device=comps.device, dtype=torch.float32).reshape(K, B, D)
            loc, theta = self._pz_params[0], self._pz_params[1]
            state = ops.lme_state(len(targets), B, comps.device)
            for k0 in range(0, K, kc):
                z, lw0 = ops.mix_ksample_logw(comps, lap, theta, kc, k0, eps=None if eps is None else eps[k0:k0 + kc],
                                              rng=self._eval_rng_state if eps is None else None,
                                              advance=k0 + kc == K, prior_loc=loc,
                                              prior_laplace=self.pz is dist.Laplace)
                rows = []
                for m in targets:
                    vae, mk = self.vaes[m], mods[m]["masks"]
                    if vae.ltype == "optimal_sigma":
                        r = torch.cat([recon_rowsum(vae.ltype, vae.dec({"latents": z[k:k + 1], "masks": mk})[0], mods[m])
                                       for k in range(kc)])
                    else:
                        # the kc * B samples as one batch (row k * B + b; the row-sum kernels pair row r with target row
                        # r % B), text masks repeated -- the form POE.objective decodes its subsets in
                        out, _ = vae.dec({"latents": z.reshape(1, kc * B, D),
                                          "masks": None if mk is None else mk.repeat(kc, 1)})
                        r = recon_rowsum(vae.ltype, out, mods[m], laplace=self._lap(vae))
                    rows.append(-r.reshape(kc, B))
                ops.lme_update(state, lw0, rows)
            out, ess = ops.lme_finish(state, K)
        return {"joint": out[0], "cond": {m: out[1 + i] for i, m in enumerate(targets)}, "ess": ess}

    # ---- latent classification ----------------------------------------------------------------
    def _sample(self, x, K=1, of=None):
        """Encoders, mixing and draws of forward(x, K), the draws through `_draw` in the reference's order -> (what
        forward() builds its distributions from, iterable of (modality, z, ...) in modality order: z is what forward()
        stores under latent_samples[modality]["latents"]).  An iterable that draws while it is read lets forward() decode
        between the draws, as the reference does.  `of` (latents_for): only that modality's z is wanted."""
        raise NotImplementedError(f"{self.modelName}: latents_for is not built for this mixer")

    def _latents_of(self, x, of):
        """forward(x)'s latent_samples[of]["latents"] without the decoders (the iterable is read to its end: its draws)"""
        return {m: z for m, z, *_ in self._sample(x, of=of)[1]}[of]

    def latents_for(self, mods, given, of=None):
        """(B, D): the latent sample that forward() stores under latent_samples["latents"] for modality `of` (default:
        the first of `given`) when only the modalities in `given` carry data -- the tensor the reference's
        classify_latents reads (eval/eval_mnistsvhn.py:24-67), K = 1 flattened.  DMVAE: its shared code.
        Encoders and the mixing only: the decoders are skipped.  Needs eval mode; runs without gradients; the noise comes
        from the evaluation generator (`_eval_rng_state`), so the training noise state, dropout counters, gradients and
        the optimiser stay as they are.  With `eps_override` the draws are consumed as forward() consumes them and the
        result equals forward()'s bit for bit."""
        names = list(self.vaes.keys())
        given = [m for m in names if m in (given or [])]
        self._need_eval("latents_for", _LATENTS)
        if not given or any(m not in mods or mods[m]["data"] is None for m in given):
            raise ValueError("latents_for: `given` must name modalities with data")
        of = given[0] if of is None else of
        if of not in names:
            raise ValueError(f"latents_for: `of` = {of!r} is not a modality of this model ({names})")
        with self._eval_noise(keep_override=True):
            z = self._latents_of(self._given_only(mods, given), of)
        return z.reshape(-1, z.shape[-1])

    def default_given(self):
        """every single modality, then all of them together"""
        names = list(self.vaes.keys())
        return [[n] for n in names] + [names]

    def probe_table(self, n_classes, n_attributes, given=None):
        """-> (given lists in modality order, their keys "+".join(names), [(s, a, C)]): probe p = s * A + a reads the
        latent matrix of subset s and label column a, with n_classes[a] classes"""
        names = list(self.vaes.keys())
        given = self.default_given() if given is None else [list(g) for g in given]
        for g in given:
            if not g or any(m not in names for m in g):
                raise ValueError(f"classify_latents: `given` entry {g} must name modalities of this model ({names})")
        given = [[m for m in names if m in g] for g in given]
        A = int(n_attributes)
        n_classes = [int(n_classes)] * A if isinstance(n_classes, int) else [int(c) for c in n_classes]
        if len(n_classes) != A:
            raise ValueError(f"classify_latents: {len(n_classes)} class counts for {A} label columns")
        for C in n_classes:
            if not 2 <= C <= ops.H.PROBE_MAX_CLASSES:
                raise ValueError(f"classify_latents: {C} classes (2 .. {ops.H.PROBE_MAX_CLASSES} are on the MI355X path)")
        return given, ["+".join(g) for g in given], [(s, a, n_classes[a]) for s in range(len(given)) for a in range(A)]

    def classify_latents(self, train, test, n_classes, given=None, epochs=30, batch_size=128, lr=1e-3, seed=0,
                         shuffle=False, init=None):
        """Latent classification (eval/eval_mnistsvhn.py:24-67): one linear probe (nn.Linear + CrossEntropyLoss + Adam)
        per (conditioning subset, label column), trained on the latents `latents_for` gives for the train set and
        scored on those of the test set.  `train` / `test`: iterables of (batch dict, labels (B,) or (B, A) ints);
        `n_classes`: an int or one per label column; `given`: modality-name lists (default_given()).
        Both sets are encoded once per subset into packed (S, N, D) device matrices; the P = S A probes of probe_table()
        train side by side, one ops.probe_train launch per epoch (`epochs` passes in minibatches of `batch_size`, in
        sequential order or, `shuffle`, in per-epoch permutations drawn from torch.Generator(seed)); the init is
        nn.Linear's from the same seed or the (W, b) pairs of `init`.
        -> {"accuracy": {(given_key, a): float}, "loss": {(given_key, a): float} (mean test cross-entropy),
            "pred": {(given_key, a): (N_test,) int32}, "train_loss": (P, steps), "state": ..., "probes": [(s, a, C)]}."""
        self._need_eval("classify_latents", _LATENTS)
        D = self.n_latents
        if D > 256:
            raise ValueError(f"classify_latents: D = {D} latent dimensions (up to 256 are on the MI355X path)")
        train, test = list(train), list(test)
        y_tr, y_te = (ops.label_matrix(s, what, "classify_latents") for s, what in ((train, "train"), (test, "test")))
        if y_tr.shape[0] != y_te.shape[0]:
            raise ValueError(f"classify_latents: {y_tr.shape[0]} train label columns, {y_te.shape[0]} test label columns")
        A = y_tr.shape[0]
        given, keys, probes = self.probe_table(n_classes, A, given)
        if len(probes) > ops.H.PROBE_MAX_PROBES:
            raise ValueError(f"classify_latents: {len(probes)} probes ({len(given)} subsets x {A} label columns); one launch "
                             f"trains up to {ops.H.PROBE_MAX_PROBES}")
        for _, a, C in probes[:A]:
            for y, what in ((y_tr, "train"), (y_te, "test")):
                if int(y[a].min()) < 0 or int(y[a].max()) >= C:
                    raise ValueError(f"classify_latents: {what} label column {a} holds labels in [{int(y[a].min())}, "
                                     f"{int(y[a].max())}], outside [0, {C})")
        for batch, _ in train + test:
            for g in given:
                if any(m not in batch or batch[m]["data"] is None for m in g):
                    raise ValueError(f"classify_latents: `given` entry {g} names a modality without data")
        if int(epochs) < 1 or int(batch_size) < 1:
            raise ValueError(f"classify_latents: epochs = {epochs}, batch_size = {batch_size}")
        z_tr = torch.stack([torch.cat([self.latents_for(b, g) for b, _ in train]) for g in given]).contiguous()
        z_te = torch.stack([torch.cat([self.latents_for(b, g) for b, _ in test]) for g in given]).contiguous()
        dev = z_tr.device
        l_tr, l_te = y_tr.to(device=dev, dtype=torch.int32), y_te.to(device=dev, dtype=torch.int32)
        N, P, Cmax = z_tr.shape[1], len(probes), max(C for _, _, C in probes)
        state = ops.probe_state(P, D, Cmax, dev, init=init, seed=seed)
        order = ops.epoch_orders(N, epochs, seed, dev, shuffle)
        spe = (N + int(batch_size) - 1) // int(batch_size)
        curve = torch.cat([ops.probe_train(state, z_tr, l_tr, probes, batch_size, e * spe, spe, lr=lr, order=order,
                                           validate=False) for e in range(int(epochs))], 1)
        pred, nll = ops.probe_eval(state, z_te, l_te, probes)
        pred, nll = pred.cpu(), nll.cpu().double()
        out = {"accuracy": {}, "loss": {}, "pred": {}, "train_loss": curve, "state": state, "probes": probes}
        for p, (s, a, _) in enumerate(probes):
            k = (keys[s], a)
            out["accuracy"][k] = int((pred[p].long() == y_te[a]).sum()) / float(y_te.shape[1])
            out["loss"][k] = float(nll[p].mean())
            out["pred"][k] = pred[p]
        return out

    # ---- latent cluster analysis ----------------------------------------------------------------
    def cluster_latents(self, batches, n_clusters, labels=None, given=None, n_init=10, max_iter=300, seed=0, init=None):
        """How the latent space clusters, per conditioning subset: k-means on the latents `latents_for` gives for every
        batch (ops.kmeans_fit: `n_init` restarts side by side from ops.kmeans_draw(N, n_clusters, n_init, seed), or from
        `init`: integer (R, C) row numbers or float64 (R, C, D) centres, for every subset), and of the restart with the
        smallest inertia the silhouette (ops.silhouette), the Calinski-Harabasz and Davies-Bouldin indices
        (ops.cluster_stats, ops.cluster_indices).  `batches`: an iterable of batch dicts; `given`: modality-name lists
        (default_given()), keys "+".join(names).
        `labels`: (N,) or (N, A) integers >= 0, ROW n the A label columns of sample n in batch order, every column with two
        values at least and ids below 64.  Per column a: ops.cluster_agreement(labels[:, a], the k-means labels) and
        label_silhouette[a] = the silhouette score of the ground-truth partition itself -- the per-label-column analysis
        the reference's utils.cluster_analysis loop asks of its analyse_clusters.
        -> {key: {"labels" (N,) int32, "centres" (C,D) float64, "inertia", "n_iter", "converged",
                  "restarts": {"inertia", "n_iter", "converged", "empty"} (R,), "silhouette": float,
                  "silhouette_samples" (N,) float64, "calinski_harabasz", "davies_bouldin": floats,
                  "agreement": {a: {"ari", "nmi", "homogeneity", "completeness", "purity"}}, "label_silhouette": {a: float}}}.
        Needs eval mode, 2 <= n_clusters <= min(64, N), N <= 16384 rows.  Runs without gradients; the draws come from the
        evaluation generator or `eps_override`: the training noise state, the dropout counters, gradients and the
        optimiser stay as they are."""
        who = "cluster_latents"
        self._need_eval(who, _LATENTS)
        names, batches, D = list(self.vaes.keys()), list(batches), self.n_latents
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        given = self.default_given() if given is None else [list(g) for g in given]
        for g in given:
            if not g or any(m not in names for m in g):
                raise ValueError(f"{who}: `given` entry {g} must name modalities of this model ({names})")
        given = [[m for m in names if m in g] for g in given]
        for batch in batches:
            for g in given:
                if any(m not in batch or batch[m]["data"] is None for m in g):
                    raise ValueError(f"{who}: `given` entry {g} names a modality without data")
        N = sum(len(b[given[0][0]]["data"]) for b in batches)
        H = ops.H
        if not 1 <= N <= H.MANIFOLD_MAX_ROWS or not 1 <= D <= H.FRECHET_MAX_F:
            raise ValueError(f"{who}: {N} rows of {D} latent dimensions (1 .. {H.MANIFOLD_MAX_ROWS} rows of 1 .. "
                             f"{H.FRECHET_MAX_F} dimensions are on the MI355X path)")
        C, n_init, max_iter = int(n_clusters), int(n_init), int(max_iter)
        if not 2 <= C <= H.CLUSTER_MAX_K or C > N:
            raise ValueError(f"{who}: n_clusters = {C} for {N} rows (2 .. {H.CLUSTER_MAX_K} clusters, at most one per row, "
                             f"are on the MI355X path)")
        if not 1 <= n_init <= H.CLUSTER_MAX_INIT or not 1 <= max_iter <= H.CLUSTER_MAX_ITER:
            raise ValueError(f"{who}: n_init = {n_init}, max_iter = {max_iter} (1 .. {H.CLUSTER_MAX_INIT} restarts of 1 .. "
                             f"{H.CLUSTER_MAX_ITER} iterations are on the MI355X path)")
        if init is not None:
            init, _ = ops.kmeans_check_init(who, init, N, D, C)
        if labels is not None:
            labels = torch.as_tensor(labels).detach().cpu()
            if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() not in (1, 2):
                raise ValueError(f"{who}: labels must be an integer (N, A) array, one row per sample")
            labels = labels.reshape(labels.shape[0], -1)
            if labels.shape[0] != N or labels.shape[1] < 1:
                raise ValueError(f"{who}: labels is {tuple(labels.shape)}, the batches hold {N} rows (one ROW of label "
                                 f"columns per sample, in batch order)")
            if int(labels.min()) < 0:
                raise ValueError(f"{who}: labels holds negative values (classes are numbered from 0)")
            for a in range(labels.shape[1]):
                if len(torch.unique(labels[:, a])) < 2 or int(labels[:, a].max()) >= H.CLUSTER_MAX_K:
                    raise ValueError(f"{who}: label column {a} takes {len(torch.unique(labels[:, a]))} value(s), the largest "
                                     f"{int(labels[:, a].max())} (its silhouette needs two classes at least; ids below "
                                     f"{H.CLUSTER_MAX_K} are on the MI355X path)")
        res = {}
        for g in given:
            z = torch.cat([self.latents_for(b, g) for b in batches]).float().contiguous()
            start = torch.from_numpy(ops.kmeans_draw(N, C, n_init, seed)) if init is None else init
            fit = ops.kmeans_fit(z, start.to(z.device), max_iter=max_iter)
            best = fit["best"]
            found = fit["labels"][best].contiguous()
            sil = ops.silhouette(z, found, C)
            idx = ops.cluster_indices(ops.cluster_stats(z, found, C))
            r = {"labels": found, "centres": fit["centres"][best], "inertia": float(fit["inertia"][best]),
                 "n_iter": int(fit["n_iter"][best]), "converged": bool(fit["converged"][best]),
                 "restarts": {k: fit[k] for k in ("inertia", "n_iter", "converged", "empty")},
                 "silhouette": sil["score"], "silhouette_samples": sil["samples"],
                 "calinski_harabasz": idx["calinski_harabasz"], "davies_bouldin": idx["davies_bouldin"],
                 "agreement": {}, "label_silhouette": {}}
            for a in range(0 if labels is None else labels.shape[1]):
                column = labels[:, a].contiguous()
                r["agreement"][a] = ops.cluster_agreement(column, found.cpu())
                r["label_silhouette"][a] = ops.silhouette(z, column.to(z.device))["score"]
            res["+".join(g)] = r
        return res

    # ---- latent density estimation ---------------------------------------------------------------
    def fit_latent_density(self, batches, n_components, given=None, held_out=None, labels=None, covariance_type="full",
                           n_init=5, max_iter=100, tol=1e-3, reg_covar=1e-6, kmeans_iter=300, seed=0):
        """Ex-post density estimation (Ghosh et al. 2020): per conditioning subset a mixture of `n_components` Gaussians
        fitted by EM to the latents `latents_for` gives for every batch (ops.gmm_fit, scikit-learn's GaussianMixture
        arithmetic in float64: `covariance_type` "full" or "diag", `tol`, `max_iter`, `reg_covar`).  `n_init` restarts run
        side by side, restart r from the labels of restart r of ops.kmeans_fit (`kmeans_iter` iterations at the most) on
        the start rows ops.kmeans_draw(N, n_components, n_init, seed); the restart with the largest lower bound is kept.
        `batches`, `held_out`: iterables of batch dicts; `given`: modality-name lists (default_given()), keys
        "+".join(names); per subset the latents of `batches` are drawn first, then those of `held_out`.
        `labels`: (N,) or (N, A) integers >= 0, ROW n the label columns of sample n in batch order.
        -> {key: {"weights" (C,), "means" (C,D), "covariances", "cholesky", "precisions_cholesky" (C,D,D) | (C,D), "log_det"
                  (C,), "covariance_type", "lower_bound", "n_iter", "converged", "restarts": {"lower_bound", "n_iter",
                  "converged", "degenerate"} (R,), "labels" (N,) int32 (the most probable component), "log_density" (N,),
                  "score": the mean log-density of the fitted latents, "held_out_score": that of the held-out latents under
                  the fit | None, "n_parameters", "bic", "aic" (ops.gmm_information), "n_rows",
                  "agreement": {a: ops.cluster_agreement(labels[:, a], the hard assignments)}}}.
        An entry is what sample_latent_density, ops.gmm_score and ops.gmm_sample take.
        Needs eval mode, 1 <= n_components <= min(64, N), N <= 16384 rows, D <= 64.  Runs without gradients; the draws come
        from the evaluation generator or `eps_override`: the training noise state, the dropout counters, gradients and the
        optimiser stay as they are."""
        who = "fit_latent_density"
        self._need_eval(who, _LATENTS)
        names, batches = list(self.vaes.keys()), list(batches)
        held_out = None if held_out is None else list(held_out)
        if not batches or (held_out is not None and not held_out):
            raise ValueError(f"{who}: `batches` is empty" if not batches else f"{who}: `held_out` is empty (None: no held-out "
                             f"score)")
        given = self.default_given() if given is None else [list(g) for g in given]
        for g in given:
            if not g or any(m not in names for m in g):
                raise ValueError(f"{who}: `given` entry {g} must name modalities of this model ({names})")
        given = [[m for m in names if m in g] for g in given]
        for batch in batches + (held_out or []):
            for g in given:
                if any(m not in batch or batch[m]["data"] is None for m in g):
                    raise ValueError(f"{who}: `given` entry {g} names a modality without data")
        N = sum(len(b[given[0][0]]["data"]) for b in batches)
        H = ops.H
        if not 1 <= N <= H.MANIFOLD_MAX_ROWS or not 1 <= self.n_latents <= H.GMM_MAX_D:
            raise ValueError(f"{who}: {N} rows of {self.n_latents} latent dimensions (1 .. {H.MANIFOLD_MAX_ROWS} rows of 1 .. "
                             f"{H.GMM_MAX_D} dimensions are on the MI355X path)")
        if held_out is not None and sum(len(b[given[0][0]]["data"]) for b in held_out) > H.MANIFOLD_MAX_ROWS:
            raise ValueError(f"{who}: `held_out` holds more than {H.MANIFOLD_MAX_ROWS} rows")
        C, n_init, kmeans_iter = int(n_components), int(n_init), int(kmeans_iter)
        if not 1 <= C <= H.CLUSTER_MAX_K or C > N:
            raise ValueError(f"{who}: n_components = {C} for {N} rows (1 .. {H.CLUSTER_MAX_K} components, at most one per row, "
                             f"are on the MI355X path)")
        if not 1 <= n_init <= H.CLUSTER_MAX_INIT or not 1 <= kmeans_iter <= H.CLUSTER_MAX_ITER:
            raise ValueError(f"{who}: n_init = {n_init}, kmeans_iter = {kmeans_iter} (1 .. {H.CLUSTER_MAX_INIT} restarts of 1 .. "
                             f"{H.CLUSTER_MAX_ITER} iterations are on the MI355X path)")
        if covariance_type not in H.GMM_COVARIANCES:
            raise ValueError(f"{who}: covariance_type = {covariance_type!r} ({', '.join(map(repr, H.GMM_COVARIANCES))})")
        reg_covar, tol, max_iter = ops.gmm_check_fit_args(who, reg_covar, tol, max_iter)
        if labels is not None:
            labels = torch.as_tensor(labels).detach().cpu()
            if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() not in (1, 2):
                raise ValueError(f"{who}: labels must be an integer (N, A) array, one row per sample")
            labels = labels.reshape(labels.shape[0], -1)
            if labels.shape[0] != N or labels.shape[1] < 1:
                raise ValueError(f"{who}: labels is {tuple(labels.shape)}, the batches hold {N} rows (one ROW of label "
                                 f"columns per sample, in batch order)")
            if int(labels.min()) < 0:
                raise ValueError(f"{who}: labels holds negative values (classes are numbered from 0)")
        res = {}
        for g in given:
            z = torch.cat([self.latents_for(b, g) for b in batches]).float().contiguous()
            z_held = None if held_out is None else torch.cat([self.latents_for(b, g) for b in held_out]).float().contiguous()
            start = torch.from_numpy(ops.kmeans_draw(N, C, n_init, seed)).to(z.device)
            km = ops.kmeans_fit(z, start, max_iter=kmeans_iter)
            fit = ops.gmm_fit(z, km["labels"], covariance_type=covariance_type, reg_covar=reg_covar, tol=tol,
                              max_iter=max_iter, n_components=C)
            best = fit["best"]
            r = {k: fit[k][best].contiguous() for k in ("weights", "means", "covariances", "cholesky", "precisions_cholesky",
                                                        "log_det", "labels", "log_density")}
            r.update({"covariance_type": covariance_type, "lower_bound": float(fit["lower_bound"][best]),
                      "n_iter": int(fit["n_iter"][best]), "converged": bool(fit["converged"][best]),
                      "restarts": {k: fit[k] for k in ("lower_bound", "n_iter", "converged", "degenerate")},
                      "score": float(fit["log_density"][best].cpu().numpy().mean()), "held_out_score": None, "n_rows": N,
                      "agreement": {}})
            r.update(ops.gmm_information(fit, N))
            if z_held is not None:
                r["held_out_score"] = ops.gmm_score(z_held, r)["score"]
            for a in range(0 if labels is None else labels.shape[1]):
                r["agreement"][a] = ops.cluster_agreement(labels[:, a].contiguous(), r["labels"].cpu())
            res["+".join(g)] = r
        return res

    def sample_latent_density(self, density, n, seed=0, u=None, eps=None):
        """n latents from a fitted density (one subset's entry of fit_latent_density) in the form the joint metrics take:
        ops.gmm_sample picks the components with `u` ((n,) float64 in [0, 1); None: numpy.random.RandomState(seed)
        .random_sample(n)) and draws z = mu_k + L_k eps (`eps` (n, D); None: the evaluation generator).
        -> {"latents" (n, D) fp32, "components" (n,) int32, "joint_eps" (n, D) fp32 = (z - loc) / scale of pz_params}:
        handed as `eps=` to joint_coherence / digit_joint_coherence or as `joint_eps=` to frechet_distances,
        manifold_metrics, kernel_distances and cross_modal_correlation, `_prior_sample` decodes these latents in place of a
        prior sample (loc + scale joint_eps = z up to one rounding).
        Needs eval mode; runs without gradients; models with private latents (DMVAE) have no joint latent to decode:
        NotImplementedError."""
        who = "sample_latent_density"
        self._need_eval(who, _GENERATIONS, shared_latents=True)
        n = int(n)
        if n < 1:
            raise ValueError(f"{who}: n = {n}")
        if not isinstance(density, dict) or not torch.is_tensor(density.get("weights")) or density["weights"].dim() != 1 or \
                not torch.is_tensor(density.get("means")) or density["means"].dim() != 2:
            raise ValueError(f"{who}: density is one subset's entry of fit_latent_density (weights (C,), means (C, D), ...)")
        D = density["means"].shape[1]
        if D != self.n_latents:
            raise ValueError(f"{who}: the density has D = {D} dimensions, the model {self.n_latents} latent dimensions")
        if u is None:
            u = torch.from_numpy(np.random.RandomState(seed).random_sample(n))
        with torch.no_grad():
            z, comp = ops.gmm_sample(density, n, u=u, eps=eps, state=self._noise_state(evaluation=True))
            loc, scale = self.pz_params
            joint_eps = ((z.double() - loc.double()) / scale.double()).float()      # (one rounding)
        return {"latents": z, "components": comp, "joint_eps": joint_eps}

    def _latent_sets(self, who, batches, given, eps, density, seed, own_checks, least, most, most_dims, why):
        """What latent_two_sample and latent_transport compare: after the guard and every argument check (`own_checks()`
        raises the metric's own refusals, after the one of empty `batches`; `least` .. `most` rows of at most `most_dims`
        dimensions, `why`: the clause on the row limit; all of it before the first encoder call), the rows Z_s latents_for
        gives for every subset over the batches (all subsets first, in the order of `given`), then N prior draws per subset
        in order from the evaluation generator (`eps`: those draws, for every subset), then, with `density`, N draws
        sample_latent_density(density[key], N, seed) per subset the fit holds.
        -> (keys, [Z_s], [prior draws], {key: density draws} | None, N)"""
        self._need_eval(who, _LATENTS)
        names, batches = list(self.vaes.keys()), list(batches)
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        own_checks()
        given = self.default_given() if given is None else [list(g) for g in given]
        for g in given:
            if not g or any(m not in names for m in g):
                raise ValueError(f"{who}: `given` entry {g} must name modalities of this model ({names})")
        given = [[m for m in names if m in g] for g in given]
        keys = ["+".join(g) for g in given]
        if not given or len(set(keys)) != len(keys):
            raise ValueError(f"{who}: the subsets {keys} (different conditioning subsets)")
        for batch in batches:
            for g in given:
                if any(m not in batch or batch[m]["data"] is None for m in g):
                    raise ValueError(f"{who}: `given` entry {g} names a modality without data")
        N, D = sum(len(b[given[0][0]]["data"]) for b in batches), self.n_latents
        if not least <= N <= most or not 1 <= D <= most_dims:
            raise ValueError(f"{who}: {N} rows of {D} latent dimensions ({least} .. {most} rows -- {why} -- of 1 .. {most_dims} "
                             f"dimensions are on the MI355X path)")
        if density is not None and (not isinstance(density, dict) or not any(k in density for k in keys)):
            raise ValueError(f"{who}: density is a result of fit_latent_density with an entry for one of {keys}")
        if eps is not None and (not torch.is_tensor(eps) or eps.numel() != N * D):
            raise ValueError(f"{who}: eps is {tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}; the (N, D) = "
                             f"({N}, {D}) prior draws")
        Z = [torch.cat([self.latents_for(b, g) for b in batches]).float().contiguous() for g in given]
        with self._eval_noise():
            priors = [self._prior_sample(N, eps, who)[0] for _ in given]
        drawn = None if density is None else {k: self.sample_latent_density(density[k], N, seed=seed)["latents"]
                                              for k in keys if k in density}
        return keys, Z, priors, drawn, N

    # ---- kernel two-sample tests of the latents ---------------------------------------------------
    def latent_two_sample(self, batches, given=None, kernel="rbf", scales=ops.MMD_SCALES, permutations=1000, seed=0,
                          eps=None, density=None):
        """How far apart are sets of latents, as distributions?  Kernel two-sample tests (Gretton et al. 2012;
        ops.mmd_two_sample, csrc/mmd.hip: unbiased MMD^2 in float64, a permutation null of `permutations` relabellings
        drawn by ops.mmd_draw(n_x, n_y, permutations, seed)).  `kernel`: "rbf" (InfoVAE's Gaussian family), "imq" (the
        WAE's inverse multiquadratics), both with the widths `scales` x the mean squared distance of the pooled sample, or
        "energy" (k = -d, the energy distance).  `batches`: an iterable of batch dicts; `given`: modality-name lists
        (default_given()), keys "+".join(names).  With Z_s the N rows latents_for gives for subset s over the batches
        (all subsets first, in the order of `given`; DMVAE: its shared code):
          "prior"[key]        Z_s against N draws of the prior p(z) = Normal(*pz_params), made after the latents, per subset
                              in order, as joint_coherence makes its latents (`eps` (N, D): those draws, for every subset)
                              -- the prior hole: which models need fit_latent_density before joint generation
          "pairs"[ka|kb]      for every unordered pair of subsets, Z_a's EVEN rows against Z_b's ODD rows -- the modality
                              gap.  The split is the point: a permutation test assumes two independent samples, and the two
                              posteriors of ONE input are not independent; the halves never share an input.
          "density"[key]      with `density` = a result of fit_latent_density: Z_s of these (held-out) batches against N
                              draws sample_latent_density(density[key], N, seed) -- did the fitted density close the gap?
                              (made after the prior draws, per subset in order; subsets the fit does not hold are left out)
        -> {"prior": {...}, "pairs": {...}, "density": {...} | None, "n": N}; every entry {"mmd2" (unbiased, may be
            negative), "p_value" = (1 + #{null >= mmd2}) / (1 + P), "null_mean", "null_std", "z", "params", "n_x", "n_y"}.
        Needs eval mode, 4 <= N <= 8192 rows, D <= 256.  Runs without gradients; the draws come from the evaluation generator
        or `eps_override`: the training noise state, the dropout counters, gradients and the optimiser stay as they are."""
        who, H = "latent_two_sample", ops.H

        def own_checks():
            if kernel not in H.MMD_KERNELS:
                raise ValueError(f"{who}: kernel = {kernel!r} (one of {', '.join(H.MMD_KERNELS)})")
            if not 0 <= int(permutations) <= H.MMD_MAX_PERMUTATIONS:
                raise ValueError(f"{who}: permutations = {int(permutations)} (0 .. {H.MMD_MAX_PERMUTATIONS} are on the MI355X "
                                 f"path)")

        keys, Z, priors, drawn, N = self._latent_sets(
            who, batches, given, eps, density, seed, own_checks, 4, H.MMD_MAX_ROWS // 2, H.MMD_MAX_D,
            "a pair keeps half of each set, a prior comparison pools twice as many")
        permutations = int(permutations)
        members = {}

        def test(X, Y):
            size = (X.shape[0], Y.shape[0])
            if size not in members:
                members[size] = torch.from_numpy(ops.mmd_draw(*size, permutations, seed)).to(X.device)
            with torch.no_grad():
                r = ops.mmd_two_sample(X, Y, member=members[size], kernel=kernel, scales=scales)
            out = {k: float(r[k]) for k in ("mmd2", "p_value", "null_mean", "null_std", "z")}
            out.update(params=r["params"], n_x=size[0], n_y=size[1])
            return out

        res = {"prior": {k: test(z, p) for k, z, p in zip(keys, Z, priors)}, "pairs": {}, "density": None, "n": N}
        for a, b in itertools.combinations(range(len(keys)), 2):
            res["pairs"][f"{keys[a]}|{keys[b]}"] = test(Z[a][0::2].contiguous(), Z[b][1::2].contiguous())
        if drawn is not None:
            res["density"] = {k: test(z, drawn[k]) for k, z in zip(keys, Z) if k in drawn}
        return res

    # ---- sliced transport distances and marginal tests of the latents ------------------------------------
    def latent_transport(self, batches, given=None, n_directions=128, seed=0, eps=None, density=None):
        """Which latent dimensions are off, and by how much?  The sets, the walk, the guards, the draw order and the keys of
        latent_two_sample; per comparison the sliced Wasserstein distances of the two sets of rows (ops.sliced_wasserstein over
        the directions ops.swd_draw(D, n_directions, seed), one set for every comparison) and the per-dimension table of
        ops.marginal_tests (csrc/swd.hip: projections on the fp64 MFMA, sorted on the device, exact for unequal sizes):
          "prior"[key]        Z_s against N draws of the prior (`eps` (N, D): those draws, for every subset)
          "pairs"[ka|kb]      Z_a's EVEN rows against Z_b's ODD rows: the Kolmogorov-Smirnov p-value assumes two independent
                              samples, and the two posteriors of ONE input are not independent; the halves never share an input
          "density"[key]      with `density` = a result of fit_latent_density: Z_s against N draws of the fitted density
        -> {"prior": {...}, "pairs": {...}, "density": {...} | None, "n": N}; every entry {"swd1": mean_l W_1, "swd2":
            sqrt(mean_l W_2^2), "max_sliced1", "max_sliced2": floats; "w1", "w2" (D,): W_1 and W_2 of every latent dimension,
            "ks" (D,): its Kolmogorov-Smirnov statistic, "ks_p" (D,): the asymptotic p-value (per dimension, uncorrected),
            float64 host tensors; "n_x", "n_y"}.
        Needs eval mode, 2 <= N <= 8192 rows, D <= 256.  Runs without gradients; the draws come from the evaluation generator
        or `eps_override`: the training noise state, the dropout counters, gradients and the optimiser stay as they are."""
        who, H = "latent_transport", ops.H

        def own_checks():
            if not 1 <= int(n_directions) <= H.SWD_MAX_DIRECTIONS:
                raise ValueError(f"{who}: n_directions = {int(n_directions)} (1 .. {H.SWD_MAX_DIRECTIONS} are on the MI355X path)")

        keys, Z, priors, drawn, N = self._latent_sets(who, batches, given, eps, density, seed, own_checks, 2, H.SWD_MAX_ROWS,
                                                      H.MMD_MAX_D, "a pair keeps half of each set")
        directions = torch.from_numpy(ops.swd_draw(self.n_latents, int(n_directions), seed)).to(Z[0].device)

        def test(X, Y):
            with torch.no_grad():
                s, t = ops.sliced_wasserstein(X, Y, directions=directions), ops.marginal_tests(X, Y)
            out = {k: float(s[k]) for k in ("swd1", "swd2", "max_sliced1", "max_sliced2")}
            out.update({k: t[k].cpu() for k in ("w1", "w2", "ks")})
            out.update(ks_p=torch.from_numpy(np.atleast_1d(t["ks_p"])), n_x=X.shape[0], n_y=Y.shape[0])
            return out

        res = {"prior": {k: test(z, p) for k, z, p in zip(keys, Z, priors)}, "pairs": {}, "density": None, "n": N}
        for a, b in itertools.combinations(range(len(keys)), 2):
            res["pairs"][f"{keys[a]}|{keys[b]}"] = test(Z[a][0::2].contiguous(), Z[b][1::2].contiguous())
        if drawn is not None:
            res["density"] = {k: test(z, drawn[k]) for k, z in zip(keys, Z) if k in drawn}
        return res

    # ---- generation coherence ------------------------------------------------------------------
    def _image_text(self, image, text):
        """names of the image and the text modality: as given, else the modality with 64 x 64 x 3 data and the other one
        (of exactly two)"""
        dims = ((64, 64, 3), (3, 64, 64))
        return self._find_modalities("coherence", (("image", image, lambda d: d in dims),
                                                   ("text", text, lambda d: d not in dims)), only_two=True)

    def cross_coherence(self, batches, classifiers, level, image=None, text=None, eps=None):
        """Cross-generation coherence of the CdSprites+ benchmark (eval/eval_cdsprites.py: calculate_cross_coherency).
        `batches`: an iterable of batch dicts holding the image and the one-hot text modality; the captions are read from
        the batches themselves (argmax of the one-hot rows over the mask's length).  `classifiers`: a
        coherence.AttributeClassifiers with one classifier per attribute of `level` (1 .. 5).  Per batch two forward()
        calls: only the text given (the decoded image is quantised to 8 bits and classified: does it show what the
        caption names?) and only the image given, text masks None so that the caption decodes at full length (its
        argmax string is compared with the caption letter by letter and attribute by attribute).
        -> {"text_image": [strict %, features %], "image_text": [strict %, features %, letters %], "per_sample": {...},
            "captions": [...], "decoded": [...]}; Image->Text strict means "every letter right", as in the reference.
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps`: a list of (B, D)
        tensors consumed in forward()'s draw order over all calls (as `eps_override`).  The training noise state, the
        dropout counters, gradients and the optimiser stay as they are."""
        self._need_eval("cross_coherence", _GENERATIONS)
        classifiers = coh.check_classifiers(classifiers, level)
        image, text = self._image_text(image, text)
        per = {"text_image_strict": [], "text_image_features": [], "image_text_strict": [], "image_text_features": [],
               "image_text_letters": []}
        captions, decoded = [], []
        with self._eval_noise(eps):
            for batch in batches:
                if any(m not in batch or batch[m]["data"] is None for m in (image, text)):
                    raise ValueError("cross_coherence: every batch must hold the image and the text modality")
                onehot, masks = batch[text]["data"], batch[text]["masks"]
                if onehot.dim() != 3:
                    raise ValueError(f"cross_coherence: the text modality must be one-hot (B,T,V), got "
                                     f"{tuple(onehot.shape)}")
                B, T, V = onehot.shape
                if V > len(coh.ALPHABET):
                    raise ValueError(f"cross_coherence: {V} symbols, the captions' alphabet has {len(coh.ALPHABET)}")
                onehot = onehot.float().contiguous()
                ids, _ = ops.text_decode_score(onehot)
                lens = (torch.full((B,), T, dtype=torch.int32, device=onehot.device) if masks is None
                        else torch.count_nonzero(masks.reshape(B, T), dim=-1).to(torch.int32))
                caps = [coh.ids_to_text(i, l) for i, l in zip(ids.cpu().tolist(), lens.cpu().tolist())]
                # text -> image
                out = self.forward(self._given_only(batch, [text]))
                x_hat = out.mods[image].decoder_dist.loc
                strict, feats, _ = coh.score_images(classifiers, level, x_hat, caps)
                per["text_image_strict"] += strict
                per["text_image_features"] += feats
                # image -> text, decoded at full length
                x = self._given_only(batch, [image])
                x[text] = dict(x[text], masks=None)
                logits = self.forward(x).mods[text].decoder_dist.loc
                logits = logits.reshape(-1, *logits.shape[-2:])[:B].float().contiguous()
                Td = logits.shape[1]
                tgt = ids[:, :Td] if Td <= T else torch.nn.functional.pad(ids, (0, Td - T))
                pred, letters = ops.text_decode_score(logits, tgt.contiguous(), lens.contiguous())
                pred, letters, lens_h = pred.cpu().tolist(), letters.cpu().tolist(), lens.cpu().tolist()
                for n in range(B):
                    dec = coh.ids_to_text(pred[n])
                    _, f, _ = coh.score_decoded_text(level, caps[n], dec)
                    per["image_text_strict"].append(int(lens_h[n] > 0 and letters[n] == lens_h[n]))
                    per["image_text_features"].append(f)
                    per["image_text_letters"].append(letters[n] / lens_h[n] if lens_h[n] else 0.0)
                    decoded.append(dec)
                captions += caps
        if not captions:
            raise ValueError("cross_coherence: `batches` is empty")
        return {"text_image": coh.mean_stats([per["text_image_strict"], per["text_image_features"]]),
                "image_text": coh.mean_stats([per["image_text_strict"], per["image_text_features"],
                                              per["image_text_letters"]]),
                "per_sample": per, "captions": captions, "decoded": decoded}

    def joint_coherence(self, classifiers, level, n=64, image=None, text=None, eps=None):
        """Joint-generation coherence (eval/eval_cdsprites.py: calculate_joint_coherency): n latents z ~ p(z) =
        Normal(*pz_params), both modalities decoded from the SAME z (text at full length), the attributes read from the
        decoded caption at their word positions ("Unknown" never matches) and compared with what the classifiers see in
        the decoded image.  (The reference draws every modality's latents on its own, from that VAE's N(0, I) --
        vae.generate_samples once per modality in trainer.save_joint_samples --, so that its image and caption do not
        share a sample; the metric's definition, one prior sample for both, is what is computed here.)
        -> {"joint": [strict %, features %], "per_sample": {...}, "decoded": [...], "attributes": [...]}.
        Needs eval mode; runs without gradients; the draw comes from the evaluation generator, or is `eps` (n, D).
        Models with private latents (DMVAE) have no joint prior sample to decode: NotImplementedError."""
        self._need_eval("joint_coherence", _GENERATIONS, shared_latents=True)
        classifiers = coh.check_classifiers(classifiers, level)
        image, text = self._image_text(image, text)
        with self._eval_noise():
            z = self._prior_sample(n, eps, "joint_coherence")
            x_hat = self.vaes[image].dec({"latents": z, "masks": None})[0]
            logits = self.vaes[text].dec({"latents": z, "masks": None})[0]
            logits = logits.reshape(-1, *logits.shape[-2:]).float().contiguous()
            pred, _ = ops.text_decode_score(logits)
            decoded = [coh.ids_to_text(p) for p in pred.cpu().tolist()]
            atts = [coh.retrieve_attributes(t, level) for t in decoded]
            strict, feats, _ = coh.score_images(classifiers, level, x_hat, atts)
        return {"joint": coh.mean_stats([strict, feats]), "per_sample": {"joint_strict": strict, "joint_features": feats},
                "decoded": decoded, "attributes": atts}

    # ---- MNIST-SVHN digit coherence ------------------------------------------------------------
    def _mnist_svhn(self, mnist, svhn):
        """names of the MNIST and the SVHN modality: as given, else the ones with 28 x 28 x 1 / 32 x 32 x 3 data"""
        return self._find_modalities("digit coherence", (("mnist", mnist, lambda d: d in ((28, 28, 1), (1, 28, 28))),
                                                         ("svhn", svhn, lambda d: d in ((32, 32, 3), (3, 32, 32)))))

    @staticmethod
    def _digit_classifiers(classifiers):
        if not isinstance(classifiers, coh.DigitClassifiers):
            raise TypeError("digit coherence: `classifiers` must be a coherence.DigitClassifiers")
        return classifiers

    def digit_cross_coherence(self, batches, classifiers, mnist=None, svhn=None, eps=None, reconstruct=False):
        """Cross-generation coherence of the MNIST-SVHN benchmark (eval/eval_mnistsvhn.py:122-154).  `batches`: an
        iterable of (batch dict, digit labels (B,) ints); `classifiers`: a trained coherence.DigitClassifiers.  Per batch
        two forward() calls: only SVHN given -- the decoded MNIST image is classified -- and only MNIST given -- the
        decoded SVHN image, permuted back to NCHW, is classified; a sample counts when the classifier reads the batch's
        label.  That is the metric as defined.  The reference's code builds the two one-modality copies of the batch and
        then forwards the FULL batch both times (lines 134-140), so that it scores reconstructions; `reconstruct=True`
        does that literally.
        -> {"svhn_mnist": %, "mnist_svhn": %, "per_sample": {"svhn_mnist": [0/1], "mnist_svhn": [0/1]},
            "pred": {"svhn_mnist": (N,) int32, "mnist_svhn": (N,) int32}, "labels": (N,) int64}.
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps`: a list of (B, D)
        tensors consumed in forward()'s draw order over all calls (as `eps_override`).  The training noise state, the
        dropout counters, gradients and the optimiser stay as they are."""
        self._need_eval("digit_cross_coherence", _GENERATIONS)
        classifiers = self._digit_classifiers(classifiers)
        mnist, svhn = self._mnist_svhn(mnist, svhn)
        batches = list(batches)
        if not batches:
            raise ValueError("digit_cross_coherence: `batches` is empty")
        y = ops.label_matrix(batches, "test", "digit_cross_coherence")
        if y.shape[0] != 1 or int(y.min()) < 0 or int(y.max()) >= 10:
            raise ValueError("digit_cross_coherence: one digit label in [0, 10) per sample")
        pred = {"svhn_mnist": [], "mnist_svhn": []}
        with self._eval_noise(eps):
            for batch, _ in batches:
                if any(m not in batch or batch[m]["data"] is None for m in (mnist, svhn)):
                    raise ValueError("digit_cross_coherence: every batch must hold the MNIST and the SVHN modality")
                B = batch[mnist]["data"].shape[0]
                out = self.forward(batch if reconstruct else self._given_only(batch, [svhn]))
                x_m = classifiers.mnist.images(out.mods[mnist].decoder_dist.loc)[:B]
                pred["svhn_mnist"].append(classifiers.predict(x_mnist=x_m)["mnist"])
                out = self.forward(batch if reconstruct else self._given_only(batch, [mnist]))
                x_s = classifiers.svhn.images(out.mods[svhn].decoder_dist.loc)[:B]
                pred["mnist_svhn"].append(classifiers.predict(x_svhn=x_s)["svhn"])
        pred = {k: torch.cat(v).cpu() for k, v in pred.items()}
        per = {k: (v.long() == y[0]).int().tolist() for k, v in pred.items()}
        return {"svhn_mnist": 100.0 * sum(per["svhn_mnist"]) / y.shape[1],
                "mnist_svhn": 100.0 * sum(per["mnist_svhn"]) / y.shape[1], "per_sample": per, "pred": pred, "labels": y[0]}

    def digit_joint_coherence(self, classifiers, n=1000, eps=None, mnist=None, svhn=None):
        """Joint-generation coherence of the MNIST-SVHN benchmark (eval/eval_mnistsvhn.py:157-180): n latents z ~ p(z) =
        Normal(*pz_params), both images decoded from the SAME z, the score is the share of samples in which the two digit
        classifiers read the same digit.  The decoded SVHN image (n,32,32,3) is permuted back to (n,3,32,32); the
        reference RESHAPES it instead (`.reshape(-1,3,32,32)`, line 170), which hands its classifier scrambled pixels --
        the metric's definition is what is computed here.
        -> {"joint": %, "per_sample": [0/1], "pred": {"mnist": (n,) int32, "svhn": (n,) int32}}.
        Needs eval mode; runs without gradients; the draw comes from the evaluation generator, or is `eps` (n, D).
        Models with private latents (DMVAE) have no joint prior sample to decode: NotImplementedError."""
        self._need_eval("digit_joint_coherence", _GENERATIONS, shared_latents=True)
        classifiers = self._digit_classifiers(classifiers)
        mnist, svhn = self._mnist_svhn(mnist, svhn)
        with self._eval_noise():
            z = self._prior_sample(n, eps, "digit_joint_coherence")
            x_m = self.vaes[mnist].dec({"latents": z, "masks": None})[0]
            x_s = self.vaes[svhn].dec({"latents": z, "masks": None})[0]
            pred = classifiers.predict(x_mnist=x_m, x_svhn=x_s)
        pred = {k: v.cpu() for k, v in pred.items()}
        same = (pred["mnist"] == pred["svhn"]).int().tolist()
        return {"joint": 100.0 * sum(same) / z.shape[1], "per_sample": same, "pred": pred}

    # ---- latent analysis ---------------------------------------------------------------------------
    def _unimodal(self, head):
        """{modality: (loc, scale, family)} of the unimodal posteriors forward() builds, from what `_sample` returns
        first"""
        raise NotImplementedError(f"{self.modelName}: analyse_latents is not built for this mixer")

    @staticmethod
    def _kl_rows(p, q):
        """torch's closed form of KL(p || q) per dimension, or NotImplementedError naming the pair"""
        if (type(p), type(q)) not in dist.kl._KL_REGISTRY:
            raise NotImplementedError(f"analyse_latents: torch has no closed form for KL({type(p).__name__} || "
                                      f"{type(q).__name__}); the reference's 100-sample estimate is not restated")
        return dist.kl_divergence(p, q)

    def analyse_latents(self, batches, perplexity=30.0, max_iter=1000, seed=123, init=None):
        """The arithmetic of the reference's analyse_data (models/trainer.py:242-272), returned as tensors; plotting stays
        with the caller.  `batches`: an iterable of batch dicts with every modality given.  Per batch the encoders, the
        mixing and the draws of forward() run (the decoders are skipped, as in latents_for); collected are, per modality,
        the tensor forward() stores under latent_samples[m]["latents"] and the (loc, scale) of its unimodal posterior.
          kl[m]      (N,D) = KL(q(z|x_m) || p(z)) per dimension, p(z) = pz(*pz_params)                  (utils.make_kl_df)
          j[m, m']   (N,D) = (KL(q_m || q_m') + KL(q_m' || q_m)) / 2 per pair of modalities, in modality order
                     with torch's closed forms on the device; a pair of families without one raises NotImplementedError
                     (the reference falls back to a 100-sample estimate there)
          tsne       one ops.tsne_embed(perplexity, max_iter, seed, init) over the concatenation of all modalities' latents
                     in modality order, as visualization.t_sne concatenates them, + "modality" (M N,) int32: the
                     modality index of every embedded point
        -> {"latents": {m: (N,D)}, "kl": {m: (N,D)}, "j": {(m, m'): (N,D)}, "tsne": {...}}.
        Two deviations from the reference: the embedding follows the exact gradient, not the Barnes-Hut approximation
        (angle 0.5) of sklearn.manifold.TSNE's default method, so that coordinates are not comparable point by point with
        the reference's plot -- the objective is --, and it embeds every sample given, not 250; DMVAE embeds its shared
        code, as in latents_for.
        Needs eval mode; runs without gradients; the noise comes from the evaluation generator, so that the training noise
        state, the dropout counters, gradients and the optimiser stay as they are.  With `eps_override` the draws are
        consumed as forward() consumes them and `latents` equals what forward() stores, bit for bit."""
        self._need_eval("analyse_latents", _LATENTS)
        names, batches = list(self.vaes.keys()), list(batches)
        # (scikit-learn's check, before anything runs: the point count is known from the batches)
        rows = sum(max((len(v["data"]) for v in b.values() if v["data"] is not None), default=0) for b in batches)
        ops.tsne_check_perplexity(perplexity, len(names) * rows)
        zs, locs, scales, family = ({m: [] for m in names} for _ in range(4))
        with self._eval_noise(keep_override=True):
            for batch in batches:
                if any(m not in batch or batch[m]["data"] is None for m in names):
                    raise ValueError("analyse_latents: every batch must hold every modality")
                head, drawn = self._sample(batch)
                for m, z, *_ in drawn:
                    zs[m].append(z.reshape(-1, z.shape[-1])[:, :self.n_latents])
                for m, (loc, scale, fam) in self._unimodal(head).items():
                    locs[m].append(loc)
                    scales[m].append(scale)
                    family[m] = fam
            if not zs[names[0]]:
                raise ValueError("analyse_latents: `batches` is empty")
            z = {m: torch.cat(zs[m]).float().contiguous() for m in names}
            q = {m: family[m](torch.cat(locs[m]), torch.cat(scales[m]), validate_args=False) for m in names}
            pz = self.pz(*self.pz_params, validate_args=False)
            kl = {m: self._kl_rows(q[m], pz) for m in names}
            j = {(a, b): 0.5 * (self._kl_rows(q[a], q[b]) + self._kl_rows(q[b], q[a]))
                 for a, b in itertools.combinations(names, 2)}
            N = z[names[0]].shape[0]
            tsne = ops.tsne_embed(torch.cat([z[m] for m in names]), perplexity=perplexity, max_iter=max_iter, seed=seed,
                                  init=init)
            tsne["modality"] = torch.arange(len(names), dtype=torch.int32, device=tsne["embedding"].device) \
                .repeat_interleave(N)
        return {"latents": z, "kl": kl, "j": j, "tsne": tsne}

    # ---- Frechet distance of generated images ------------------------------------------------------
    def frechet_distances(self, batches, features, n_joint=0, eps=None, joint_eps=None):
        """Frechet distance d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 between the features of real and of
        generated images: the arithmetic of the reference's calculate_frechet_distance (eval/fid_score.py:203-257), in
        float64 on the device (ops.frechet_*; csrc/frechet.hip).  `batches`: an iterable of batch dicts; `features`:
        {modality: callable}, each mapping a tensor to (rows, F) float features on the device -- coherence.
        attribute_features(classifier), DigitClassifier.features, or a module of the caller's (with InceptionV3's pooled
        features this is FID proper).  A callable receives batch[m]["data"] for the real rows and decoder_dist.loc for
        generated ones; of the rows it returns for a generation, the first B (the batch's rows) are folded, as the digit
        coherence reads them.  Per modality m in `features`, streaming moment states (memory does not grow with the rows):
          real       every batch's data, folded first;
          recon      forward() of the full batch;
          cross[g]   forward() with only modality g given, for every other modality g;
          joint      n_joint > 0: the decoder output of n_joint latents z ~ p(z) (`joint_eps` (n_joint, D) replaces the draw).
        Per batch forward() runs on the full batch, then once per modality g in modality order.
        -> {m: {"recon": d^2, "cross": {g: d^2}, "joint": d^2 | None, "n": real rows, "F": F,
                "sweeps": {"recon": (s1, s2), "cross": {g: (s1, s2)}, "joint": (s1, s2) | None}}}, distances as floats, the
        sweeps those of the two Jacobi eigendecompositions of a distance.
        Deviations from the reference: the square root is taken through two symmetric eigendecompositions (S1 = V L V^T,
        then R S2 R^T with R = L^1/2 V^T) instead of a Schur sqrtm of the non-symmetric product S1 S2; its fallback of
        adding 1e-6 to both diagonals applies only when sqrtm returns non-finite values, which this route never does, and
        is not restated, nor is its check of the imaginary part; the feature extractor is the caller's (InceptionV3's
        weights cannot be shipped).
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps`: a list of (B, D)
        tensors consumed in forward()'s draw order over all calls (as `eps_override`).  The training noise state, the
        dropout counters, gradients and the optimiser stay as they are."""
        states = {}

        def fold(m, key, f):
            if (m, key) not in states:
                states[(m, key)] = ops.frechet_state(f.shape[1], f.device)
            ops.frechet_update(states[(m, key)], f)

        def rows_ok(rows, n_joint):
            if rows < 2 or n_joint == 1:
                raise ValueError(f"frechet_distances: {rows} real rows, n_joint = {n_joint} (a covariance needs two rows)")

        mods, dims = self._walk_generations("frechet_distances", batches, features, n_joint, eps, joint_eps, rows_ok, fold)
        with torch.no_grad():
            res = {}
            for m in mods:
                n, mu, sigma = ops.frechet_moments(states[(m, "real")])
                r = {"recon": None, "cross": {}, "joint": None, "n": n, "F": dims[m],
                     "sweeps": {"recon": None, "cross": {}, "joint": None}}
                for (mm, key), st in states.items():
                    if mm != m or key == "real":
                        continue
                    _, mu_g, sigma_g = ops.frechet_moments(st)
                    d = ops.frechet_distance(mu, sigma, mu_g, sigma_g)
                    if isinstance(key, tuple):
                        r["cross"][key[1]], r["sweeps"]["cross"][key[1]] = float(d["distance"]), d["sweeps"]
                    else:
                        r[key], r["sweeps"][key] = float(d["distance"]), d["sweeps"]
                res[m] = r
        return res

    # ---- precision, recall, density and coverage of generated images -------------------------------
    def manifold_metrics(self, batches, features, k=5, n_joint=0, eps=None, joint_eps=None):
        """k-nearest-neighbour manifold estimates between the features of real and of generated images: improved precision
        and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) -- what a Frechet distance cannot
        tell apart: poor samples (low precision, density) from samples that cover part of the data (low recall, coverage).
        Squared distances in float64 on the device (ops.manifold_prdc; csrc/manifold.hip); with R the real rows, G a
        generated set of M rows and rad^2_X[i] the k-th smallest d^2 from row i of X to the other rows of X:
          precision = mean_j [some i: d^2(G_j, R_i) <= rad^2_R[i]]      recall = mean_i [some j: d^2(R_i, G_j) <= rad^2_G[j]]
          density   = #{(i, j): d^2(G_j, R_i) <= rad^2_R[i]} / (k M)    coverage = mean_i [min_j d^2(R_i, G_j) <= rad^2_R[i]]
        `batches`, `features`, `n_joint`, `eps`, `joint_eps`, the sets (real, recon, cross[g], joint) and the order of the
        forward() calls are those of frechet_distances; the fp32 feature rows of every set are kept until the walk ends.
        -> {m: {"recon": {"precision", "recall", "density", "coverage"}, "cross": {g: {...}}, "joint": {...} | None,
                "n": real rows, "F": F, "k": k}}, floats.
        Needs eval mode, k + 1 .. 16384 real rows, n_joint = 0 or >= k + 1, 1 <= k <= 16; runs without gradients; the
        training noise state, the dropout counters, gradients and the optimiser stay as they are."""
        k, top_k, top_rows = int(k), ops.H.MANIFOLD_MAX_K, ops.H.MANIFOLD_MAX_ROWS
        sets = {}

        def rows_ok(rows, n_joint):
            if not 1 <= k <= top_k:
                raise ValueError(f"manifold_metrics: k = {k} neighbours (1 .. {top_k} are on the MI355X path)")
            if not k + 1 <= rows <= top_rows or 0 < n_joint < k + 1 or n_joint > top_rows:
                raise ValueError(f"manifold_metrics: {rows} real rows, n_joint = {n_joint} (the k-th neighbour needs k + 1 = "
                                 f"{k + 1} rows in a set; up to {top_rows} are on the MI355X path)")

        def keep_rows(f):      # a copy: a kept view would hold the extractor's whole output (rows beyond B) until the end
            return f.detach().to(torch.float32, copy=True)

        mods, dims = self._walk_generations("manifold_metrics", batches, features, n_joint, eps, joint_eps, rows_ok,
                                            lambda m, key, f: sets.setdefault((m, key), []).append(keep_rows(f)))
        names = ("precision", "recall", "density", "coverage")
        res = {}
        with torch.no_grad():
            for m in mods:
                real = torch.cat(sets[(m, "real")])
                r = {"recon": None, "cross": {}, "joint": None, "n": real.shape[0], "F": dims[m], "k": k}
                for (mm, key), rows in sets.items():
                    if mm != m or key == "real":
                        continue
                    out = ops.manifold_prdc(real, torch.cat(rows), k=k)
                    out = {name: out[name] for name in names}
                    if isinstance(key, tuple):
                        r["cross"][key[1]] = out
                    else:
                        r[key] = out
                res[m] = r
        return res

    # ---- kernel inception distance of generated images ------------------------------------------------
    def kernel_distances(self, batches, features, subsets=100, subset_size=1000, seed=0, n_joint=0, eps=None, joint_eps=None):
        """Kernel inception distance (Binkowski et al. 2018) between the features of real and of generated images: the
        unbiased estimate of the squared maximum mean discrepancy under the polynomial kernel k(x, y) = (x . y / F + 1)^3,
        in float64 on the device (ops.kernel_inception_distance; csrc/kid.hip).  With R the real rows and G a generated set,
        per subset s of m = min(subset_size, |R|, |G|) rows of each, drawn without replacement:
          mmd2[s] = sum_{i != j} k(r_i, r_j) / (m (m - 1)) + sum_{i != j} k(g_i, g_j) / (m (m - 1)) - 2 sum_{i, j} k(r_i, g_j) / m^2
          kid = mean_s mmd2[s]      std = the standard deviation of mmd2 over the subsets (divisor `subsets`)
        Unlike the Frechet distance the estimate is unbiased at any set size -- models evaluated on different numbers of
        rows can be compared -- and `std` is its error bar; a negative value is a legitimate estimate and is kept.
        `batches`, `features`, `n_joint`, `eps`, `joint_eps`, the sets (real, recon, cross[g], joint) and the order of the
        forward() calls are those of frechet_distances; the fp32 feature rows of every set are kept until the walk ends.
        Every generated set is compared with the real rows on subsets drawn from a fresh numpy.random.RandomState(seed)
        (ops.kid_draw).
        -> {m: {"recon": {"kid", "std"}, "cross": {g: {"kid", "std"}}, "joint": {"kid", "std"} | None, "n": real rows,
                "F": F, "subsets": subsets, "m": {"recon" | "from_<g>" | "joint": the rows per subset of that set}}}, floats.
        Deviations from the usual KID: no Inception network -- the feature extractor is the caller's, as in
        frechet_distances (with InceptionV3's pooled features this is KID proper); the subsets come from numpy's legacy
        generator in the order stated in ops.kid_draw, not from any other implementation's stream.
        Needs eval mode, 2 real rows at least, n_joint = 0 or >= 2, 1 <= subsets <= 1024; runs without gradients; the
        training noise state, the dropout counters, gradients and the optimiser stay as they are."""
        subsets, subset_size, top = int(subsets), int(subset_size), ops.H.KID_MAX_SUBSETS
        sets = {}

        def rows_ok(rows, n_joint):
            if not 1 <= subsets <= top or subset_size < 2:
                raise ValueError(f"kernel_distances: {subsets} subsets of {subset_size} rows (1 .. {top} subsets of two rows "
                                 f"at least are on the MI355X path)")
            if rows < 2 or n_joint == 1:
                raise ValueError(f"kernel_distances: {rows} real rows, n_joint = {n_joint} (the unbiased estimate needs two "
                                 f"rows of each set)")

        def keep_rows(f):      # a copy: a kept view would hold the extractor's whole output (rows beyond B) until the end
            return f.detach().to(torch.float32, copy=True)

        mods, dims = self._walk_generations("kernel_distances", batches, features, n_joint, eps, joint_eps, rows_ok,
                                            lambda m, key, f: sets.setdefault((m, key), []).append(keep_rows(f)))
        res = {}
        with torch.no_grad():
            for m in mods:
                real = torch.cat(sets[(m, "real")])
                r = {"recon": None, "cross": {}, "joint": None, "n": real.shape[0], "F": dims[m], "subsets": subsets, "m": {}}
                for (mm, key), rows in sets.items():
                    if mm != m or key == "real":
                        continue
                    out = ops.kernel_inception_distance(real, torch.cat(rows), subsets=subsets, subset_size=subset_size,
                                                        seed=seed)
                    pair = {"kid": float(out["kid"]), "std": float(out["std"])}
                    if isinstance(key, tuple):
                        r["cross"][key[1]], r["m"]["from_{}".format(key[1])] = pair, out["m"]
                    else:
                        r[key], r["m"][key] = pair, out["m"]
                res[m] = r
        return res

    # ---- sliced Wasserstein distance of generated rows ----------------------------------------------------
    def sliced_distances(self, batches, features, n_directions=128, seed=0, n_joint=0, eps=None, joint_eps=None):
        """Sliced Wasserstein distances (Rabin et al. 2011; Bonneel et al. 2015; max-sliced: Deshpande et al. 2019) between
        the features of real and of generated rows, in float64 on the device (ops.sliced_wasserstein; csrc/swd.hip): a
        transport distance with no kernel width and no moment estimate, exact for sets of different sizes.
        `batches`, `features`, `n_joint`, `eps`, `joint_eps`, the sets (real, recon, cross[g], joint) and the order of the
        forward() calls are those of frechet_distances; the fp32 rows of every set are kept until the walk ends.
        `features[m]` may be `lambda x: x.flatten(1)`: the distance is then taken on the raw pixels and needs no classifier, no
        labels and no weights -- which is the point.  The directions are ops.swd_draw(F, n_directions, seed), one set for every
        modality of one feature width.
        -> {m: {"recon": {...}, "cross": {g: {...}}, "joint": {...} | None, "n": real rows, "F": F}}, every {...} = {"swd1":
            mean_l W_1, "swd2": sqrt(mean_l W_2^2), "max_sliced1": max_l W_1, "max_sliced2": sqrt(max_l W_2^2), floats; "n":
            the rows of the generated set}.
        Needs eval mode, at most 8192 rows per set, F <= 16384, 1 <= n_directions <= 1024; runs without gradients; the training
        noise state, the dropout counters, gradients and the optimiser stay as they are."""
        who, H = "sliced_distances", ops.H
        n_directions, sets, drawn = int(n_directions), {}, {}

        def rows_ok(rows, n_joint):
            if not 1 <= n_directions <= H.SWD_MAX_DIRECTIONS:
                raise ValueError(f"{who}: n_directions = {n_directions} (1 .. {H.SWD_MAX_DIRECTIONS} are on the MI355X path)")
            if not 1 <= rows <= H.SWD_MAX_ROWS or n_joint > H.SWD_MAX_ROWS:
                raise ValueError(f"{who}: {rows} real rows, n_joint = {n_joint} (1 .. {H.SWD_MAX_ROWS} rows per set are on the "
                                 f"MI355X path)")

        def keep_rows(f):      # a copy: a kept view would hold the extractor's whole output (rows beyond B) until the end
            return f.detach().to(torch.float32, copy=True)

        mods, dims = self._walk_generations(who, batches, features, n_joint, eps, joint_eps, rows_ok,
                                            lambda m, key, f: sets.setdefault((m, key), []).append(keep_rows(f)))
        res = {}
        with torch.no_grad():
            for m in mods:
                real, F = torch.cat(sets[(m, "real")]), dims[m]
                if not 1 <= F <= H.SWD_MAX_F:
                    raise ValueError(f"{who}: the extractor of {m!r} returned F = {F} features (1 .. {H.SWD_MAX_F} are on the "
                                     f"MI355X path)")
                if F not in drawn:
                    drawn[F] = torch.from_numpy(ops.swd_draw(F, n_directions, seed)).to(real.device)
                r = {"recon": None, "cross": {}, "joint": None, "n": real.shape[0], "F": F}
                for (mm, key), rows in sets.items():
                    if mm != m or key == "real":
                        continue
                    gen = torch.cat(rows)
                    out = ops.sliced_wasserstein(real, gen, directions=drawn[F])
                    entry = {k: float(out[k]) for k in ("swd1", "swd2", "max_sliced1", "max_sliced2")}
                    entry["n"] = gen.shape[0]
                    if isinstance(key, tuple):
                        r["cross"][key[1]] = entry
                    else:
                        r[key] = entry
                res[m] = r
        return res

    # ---- cross-modal correlation of generations -------------------------------------------------------
    def cross_modal_correlation(self, fit_batches, batches, features, k, ridge=1e-12, n_joint=0, eps=None, joint_eps=None):
        """Canonical-correlation score of generations (Shi et al. 2019, the coherence measure of image-caption models such
        as CUB): the one coherence metric that needs neither labels nor a classifier.  The arithmetic of the reference's
        cca (eval/mnistsvhn_helper.py:26-78) in float64 on the device (ops.cca_fit, ops.cca_score; csrc/cca.hip).
        `features`: {modality: callable -> (rows, o_m) float features}, two modalities at least (for captions
        coherence.SentenceFeatures); a callable receives batch[m]["data"] for real rows and decoder_dist.loc for generated
        ones, of whose rows the first B (the batch's) are read.
          Fit    the real rows of `fit_batches`: every modality's features side by side in model order, streamed into one
                 moment state (memory does not grow with the rows), then multi-view CCA with `k` joint dimensions.
          Score  over `batches`, per row the cosine of the two projected, centred features; a (sum, rows) pair per key in
                 double:
                   real[(a, b)]    real a against real b: the ceiling the data itself reaches
                   recon[(a, b)]   both from forward() of the full batch
                   cross[(g, m)]   real g against m generated from g alone, every ordered pair
                   joint[(a, b)]   n_joint > 0 only: both decoded from the same n_joint latents z ~ p(z) (`joint_eps`
                                   (n_joint, D) replaces the draw)
                 (a, b) run over the pairs of `features` in model order, a before b.  With more than two views a pair
                 uses its two blocks of the joint projections, as the reference's torch.split does.
        Per batch forward() runs on the full batch, then once per modality g of `features` in model order.
        -> {"real", "recon", "cross"[, "joint"]: {pair: mean cosine, a float}, "correlations": [k floats], "k", "n_fit",
            "widths": {m: o_m}, "condition": {m: lambda_min / lambda_max of m's covariance + ridge I},
            "sweeps": {"views": {m: sweeps}, "joint": sweeps of the whitened matrix}}.
        The widths together may not exceed 2048, the eigensolver's limit (a 2048-wide ResNet feature beside a 300-wide
        sentence feature is outside it: reduce the image feature first).  Deviations from the reference: `k` is required
        (its Otsu threshold for k=None is not restated); the covariances are float64 from the float32 features.
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps` (as frechet_distances).
        The training noise state, the dropout counters, gradients and the optimiser stay as they are."""
        who = "cross_modal_correlation"
        n_joint = int(n_joint)
        self._need_eval(who, _GENERATIONS, shared_latents=n_joint > 0)
        names, fit_batches, batches = list(self.vaes.keys()), list(fit_batches), list(batches)
        if not fit_batches or not batches:
            raise ValueError(f"{who}: `fit_batches` and `batches` must not be empty")
        if not isinstance(features, dict) or any(m not in names or not callable(f) for m, f in features.items()):
            raise ValueError(f"{who}: `features` maps modalities of this model ({names}) to callables")
        mods = [m for m in names if m in features]
        if not 2 <= len(mods) <= ops.H.CCA_MAX_VIEWS:
            raise ValueError(f"{who}: `features` names {len(mods)} modalities (a correlation needs 2 .. "
                             f"{ops.H.CCA_MAX_VIEWS} views)")
        for batch in fit_batches + batches:
            if any(m not in batch or batch[m]["data"] is None for m in names):
                raise ValueError(f"{who}: every batch must hold every modality (a modality without data)")
        k, ridge = int(k), float(ridge)
        if not 1 <= k <= ops.H.CCA_MAX_K or not ridge > 0.0 or n_joint < 0:
            raise ValueError(f"{who}: k = {k} (1 .. {ops.H.CCA_MAX_K}), ridge = {ridge} (positive), n_joint = {n_joint}")
        n_fit = sum(len(b[mods[0]]["data"]) for b in fit_batches)
        if n_fit < 2:
            raise ValueError(f"{who}: {n_fit} rows to fit (a covariance needs two rows)")
        dims = {}

        def feat(m, x, keep=None):
            f = features[m](x)
            if not torch.is_tensor(f) or f.dim() != 2 or not f.is_floating_point():
                raise ValueError(f"{who}: the extractor of {m!r} must return float (rows, o) features")
            if dims.setdefault(m, f.shape[1]) != f.shape[1]:
                raise ValueError(f"{who}: the extractor of {m!r} returned o = {f.shape[1]} after o = {dims[m]}")
            return f.float() if keep is None else f[:keep].float()

        pairs = list(itertools.combinations(mods, 2))
        sums = {}

        def score(table, key, fa, fb):
            a, b = key
            _, s = ops.cca_score(fa, fb, fit["means"][at[a]], fit["means"][at[b]], fit["projections"][at[a]],
                                 fit["projections"][at[b]])
            old = sums.get((table, key))
            sums[(table, key)] = (s if old is None else old[0] + s, fa.shape[0] + (0 if old is None else old[1]))

        with self._eval_noise(eps):
            state = None
            for batch in fit_batches:
                rows = torch.cat([feat(m, batch[m]["data"]) for m in mods], dim=1)
                if state is None:
                    widths = ops.cca_check_widths(who, [dims[m] for m in mods], rows.shape[1])
                    if k > min(widths):
                        raise ValueError(f"{who}: k = {k} joint dimensions, the narrowest view has {min(widths)} features")
                    state = ops.frechet_state(rows.shape[1], rows.device)
                ops.frechet_update(state, rows)
            n_fit, mu, sigma = ops.frechet_moments(state)
            fit = ops.cca_fit(mu, sigma, widths, k, ridge)
            at = {m: i for i, m in enumerate(mods)}
            for batch in batches:
                B = len(batch[mods[0]]["data"])
                real = {m: feat(m, batch[m]["data"]) for m in mods}
                for a, b in pairs:
                    score("real", (a, b), real[a], real[b])
                out = self.forward(batch)
                recon = {m: feat(m, out.mods[m].decoder_dist.loc, B) for m in mods}
                for a, b in pairs:
                    score("recon", (a, b), recon[a], recon[b])
                for g in mods:
                    out = self.forward(self._given_only(batch, [g]))
                    for m in mods:
                        if m != g:
                            score("cross", (g, m), real[g], feat(m, out.mods[m].decoder_dist.loc, B))
            if n_joint > 0:
                z = self._prior_sample(n_joint, joint_eps, who)
                joint = {m: feat(m, self.vaes[m].dec({"latents": z, "masks": None})[0]) for m in mods}
                for a, b in pairs:
                    score("joint", (a, b), joint[a], joint[b])
            res = {t: {} for t in ("real", "recon", "cross") + (("joint",) if n_joint > 0 else ())}
            for (table, key), (s, rows) in sums.items():
                res[table][key] = float(s) / rows
        res.update({"correlations": fit["correlations"].tolist(), "k": k, "n_fit": n_fit, "widths": dict(zip(mods, widths)),
                    "condition": dict(zip(mods, fit["condition"])),
                    "sweeps": {"views": dict(zip(mods, fit["sweeps"]["views"])), "joint": fit["sweeps"]["joint"]}})
        return res

    # ---- disentanglement of the latent code ----------------------------------------------------------
    def _joint_posterior(self, head):
        """(loc, scale) of the joint posterior forward() builds when it is ONE Gaussian (the product of experts of poe and
        dmvae), from what `_sample` returns first; None where the joint is a mixture (moe, mopoe): out of scope"""
        return None

    def _walk_posteriors(self, batches):
        """Inside `_eval_noise`: per batch the encoders, the mixing and the draws of forward() (the decoders are skipped)
        -> ({key: loc (N,D) fp32}, {key: scale (N,D) fp32}, {key: family}) over the rows of all batches, D = n_latents (the
        first columns: DMVAE's shared code); keys: every modality's unimodal posterior and, where `_joint_posterior`
        gives one Gaussian, "joint".  What disentanglement and cross_modal_retrieval read."""
        locs, scales, family = {}, {}, {}
        for batch in batches:
            head, drawn = self._sample(batch)
            for _ in drawn:      # (read to its end: the draws forward() takes)
                pass
            found = dict(self._unimodal(head))
            joint = self._joint_posterior(head)
            if joint is not None:
                found["joint"] = (joint[0], joint[1], dist.Normal)
            for key, (loc, scale, fam) in found.items():
                locs.setdefault(key, []).append(loc)
                scales.setdefault(key, []).append(scale)
                family[key] = fam
        D = self.n_latents

        def rows(ts):
            return torch.cat([t.reshape(-1, t.shape[-1])[:, :D] for t in ts]).float().contiguous()
        return {k: rows(v) for k, v in locs.items()}, {k: rows(v) for k, v in scales.items()}, family

    def disentanglement(self, batches, labels=None, eps=None, chunks=0):
        """Disentanglement of the latent code, per posterior: the decomposition of the ELBO's KL term into index-code mutual
        information, total correlation and dimension-wise KL, and the mutual information gap against labelled generative
        factors (both Chen et al. 2018), from the aggregate posterior q(z) = (1/N) sum_m q(z | x_m) evaluated at one draw
        per sample in float64 on the device (ops.aggregate_posterior; csrc/aggpost.hip).
        `batches`: an iterable of batch dicts with every modality given.  Per batch the encoders, the mixing and the draws
        of forward() run (the decoders are skipped, as in analyse_latents); collected are the (loc, scale, family) of every
        modality's unimodal posterior (the first n_latents columns: DMVAE's shared code) and, for poe and dmvae, of the
        product of experts (key "joint"; the mixture joints of moe and mopoe are not covered).  Per key, over the N rows
        of all batches: e (N,D) of the key's family from the evaluation generator, or `eps[key]`; z = loc + scale e;
        lpz = sum_d log p(z_d) under pz(*pz_params); then ops.aggregate_posterior, ops.elbo_decomposition and, with
        labels, ops.mutual_information_gap.
        `labels`: (N, K) integers >= 0, ROW n the K generative factors of sample n in batch order (a (N,) vector is one
        factor), K <= 8; without labels the entries mig, per_factor and mi_table are absent.
        -> {key: {"mi", "tc", "dwkl", "kl" (0-d float64), "mig" (0-d), "per_factor" (K,), "mi_table" (K,D), "h_z" (D,),
                  "z", "loc", "scale" (N,D) fp32}}, keys in modality order, then "joint".
        Needs eval mode, N <= 16384 rows, D <= 256; with labels D >= 2 and every factor taking two values at least.  Runs
        without gradients; the draws of the walk come from the evaluation generator: the training noise state, the dropout
        counters, `eps_override`, gradients and the optimiser stay as they are."""
        who = "disentanglement"
        self._need_eval(who, _LATENTS)
        names, batches, D = list(self.vaes.keys()), list(batches), self.n_latents
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        for batch in batches:
            if any(m not in batch or batch[m]["data"] is None for m in names):
                raise ValueError(f"{who}: every batch must hold every modality")
        N = sum(len(b[names[0]]["data"]) for b in batches)
        if not 1 <= N <= ops.H.AGGPOST_MAX_ROWS or not 1 <= D <= ops.H.AGGPOST_MAX_DIM:
            raise ValueError(f"{who}: {N} rows of {D} latent dimensions (1 .. {ops.H.AGGPOST_MAX_ROWS} rows of 1 .. "
                             f"{ops.H.AGGPOST_MAX_DIM} dimensions are on the MI355X path)")
        if int(chunks) < 0:
            raise ValueError(f"{who}: chunks = {chunks} (0: the default plan, or a positive number of chunks)")
        if labels is not None:
            labels = torch.as_tensor(labels).detach()
            if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() not in (1, 2):
                raise ValueError(f"{who}: labels must be an integer (N, K) array, one row per sample")
            labels = labels.reshape(labels.shape[0], -1)
            if labels.shape[0] != N or not 1 <= labels.shape[1] <= ops.H.AGGPOST_MAX_FACTORS:
                raise ValueError(f"{who}: labels is {tuple(labels.shape)}, the batches hold {N} rows (one ROW of 1 .. "
                                 f"{ops.H.AGGPOST_MAX_FACTORS} factors per sample, in batch order)")
            if int(labels.min()) < 0:
                raise ValueError(f"{who}: labels holds negative values (classes are numbered from 0)")
            if D < 2:
                raise ValueError(f"{who}: the mutual information gap needs D >= 2 latent dimensions (D = {D})")
            for k in range(labels.shape[1]):
                if len(torch.unique(labels[:, k])) < 2:
                    raise ValueError(f"{who}: factor {k} of labels takes a single value (H(v) = 0: the gap is not defined)")
            labels = labels.t().contiguous()
        eps = dict(eps or {})
        for key, e in eps.items():
            if key not in names + ["joint"] or not torch.is_tensor(e) or tuple(e.shape) != (N, D):
                raise ValueError(f"{who}: eps maps {names + ['joint']} to ({N}, {D}) tensors (entry {key!r})")
        with self._eval_noise():
            locs, scales, family = self._walk_posteriors(batches)
            if "joint" in eps and "joint" not in locs:
                raise ValueError(f"{who}: eps['joint'] given, but the joint posterior of {self.modelName} is not one Gaussian")
            pz_loc, pz_scale = (p.detach().double() for p in self.pz_params)
            res = {}
            for key in names + (["joint"] if "joint" in locs else []):
                loc, scale = locs[key], scales[key]
                laplace = family[key] is dist.Laplace
                if key in eps:
                    e = eps[key].to(device=loc.device, dtype=torch.float32)
                else:
                    e = (ops.rand_laplace if laplace else ops.randn)((N, D), self._noise_state())
                z = (loc + scale * e).contiguous()
                lpz = self.pz(pz_loc, pz_scale, validate_args=False).log_prob(z.double()).sum(1)
                lab = None if labels is None else labels.to(z.device)
                agg = ops.aggregate_posterior(z, loc, scale, laplace=laplace, labels=lab, chunks=chunks)
                r = dict(ops.elbo_decomposition(agg, lpz))
                r["h_z"] = -agg["marginal"].mean(0)
                if lab is not None:
                    gap = ops.mutual_information_gap(agg, lab)
                    r.update(mig=gap["mig"], per_factor=gap["per_factor"], mi_table=gap["mi"], h_z=gap["h_z"])
                r.update(z=z, loc=loc, scale=scale)
                res[key] = r
        return res

    # ---- cross-modal retrieval of latents -----------------------------------------------------------------
    def cross_modal_retrieval(self, batches, metric="l2", ks=(1, 5, 10), keep=10, labels=None, use="posterior", given=None):
        """Are the modalities aligned in the latent space, sample by sample?  For every ordered pair (a, b) of sets, query
        row n of a retrieves from the N rows of b; its partner is row n of b, the same sample (ops.retrieval_ranks;
        csrc/retrieval.hip: float64 distances, exact ranks).  No labels, no classifier, no weights.
        `batches`: an iterable of batch dicts.
        use "posterior": the sets are the modalities' unimodal posteriors (loc, scale), collected as disentanglement
          collects them (deterministic: no draw enters; every batch must hold every modality); metric "l2" / "cosine" on
          the means, "w2" / "skl" (squared 2-Wasserstein, symmetrised KL) on the Gaussians -- a family other than Normal
          raises NotImplementedError there.  Keys are the modality names.
        use "sample": the sets are latents_for(batch, g) for g in `given` (default: every single modality; keys
          "+".join(g)); "l2" / "cosine" only.  The draws come from the evaluation generator or `eps_override`.
        `labels`: (N,) or (N, A) integers >= 0, ROW n the label columns of sample n in batch order: per column, the share of
        a query's k nearest rows that carry its label and the hit rate (ops.retrieval_label_precision, k <= keep).
        Ranks are PESSIMISTIC (ops.retrieval_summary): rank = 1 + nearer rows + rows exactly as near, so collapsed
        posteriors, all equidistant, score rank N and recall 0, not rank 1.
        -> {"a->b": {"recall@k", "chance@k", "median_rank", "mean_rank", "mrr", "normalised_rank", "tied_rows", "n",
                     "d_match" (N,) float64, "rank" (N,) int32, "nn_idx" (N, keep) int32,
                     "label_precision": {column: {k: {"precision", "hit"}}} with labels}, ...,
            "mean": the summary fields averaged over the pairs}.
        Needs eval mode, N <= 16384 rows, D <= 256, 2 .. 16 sets, keep <= 16.  Runs without gradients: the training noise
        state, the dropout counters, gradients and the optimiser stay as they are (use "posterior": `eps_override` too)."""
        who = "cross_modal_retrieval"
        self._need_eval(who, _LATENTS)
        names, batches, D, H = list(self.vaes.keys()), list(batches), self.n_latents, ops.H
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        if metric not in H.RETRIEVAL_METRICS:
            raise ValueError(f"{who}: metric = {metric!r} ({', '.join(H.RETRIEVAL_METRICS)})")
        if use not in ("posterior", "sample"):
            raise ValueError(f"{who}: use = {use!r} ('posterior' or 'sample')")
        if use == "sample" and metric in ("w2", "skl"):
            raise ValueError(f"{who}: metric {metric!r} compares posteriors; samples are compared by 'l2' or 'cosine'")
        if use == "posterior" and given is not None:
            raise ValueError(f"{who}: `given` selects the sets of use='sample'; the posteriors are the modalities' own")
        given = [[m] for m in names] if given is None else [list(g) for g in given]
        for g in given:
            if not g or any(m not in names for m in g):
                raise ValueError(f"{who}: `given` entry {g} must name modalities of this model ({names})")
        given = [[m for m in names if m in g] for g in given]
        keys = names if use == "posterior" else ["+".join(g) for g in given]
        need = [names] if use == "posterior" else given
        for batch in batches:
            for g in need:
                if any(m not in batch or batch[m]["data"] is None for m in g):
                    raise ValueError(f"{who}: every batch must hold every modality" if use == "posterior" else
                                     f"{who}: `given` entry {g} names a modality without data")
        N, keep, ks = sum(len(b[need[0][0]]["data"]) for b in batches), int(keep), [int(k) for k in ks]
        if len(set(keys)) != len(keys) or not 2 <= len(keys) <= H.RETRIEVAL_MAX_SETS:
            raise ValueError(f"{who}: the sets {keys} (2 .. {H.RETRIEVAL_MAX_SETS} different sets are on the MI355X path)")
        if not 1 <= N <= H.RETRIEVAL_MAX_ROWS or not 1 <= D <= H.RETRIEVAL_MAX_DIM or not 0 <= keep <= H.RETRIEVAL_MAX_KEEP:
            raise ValueError(f"{who}: {N} rows of {D} latent dimensions, keep = {keep} (1 .. {H.RETRIEVAL_MAX_ROWS} rows of "
                             f"1 .. {H.RETRIEVAL_MAX_DIM} dimensions and 0 .. {H.RETRIEVAL_MAX_KEEP} neighbours are on the "
                             f"MI355X path)")
        if not ks or min(ks) < 1 or len(set(ks)) != len(ks):
            raise ValueError(f"{who}: ks = {ks} (different positive numbers of neighbours)")
        if labels is not None:
            labels = torch.as_tensor(labels).detach().cpu()
            if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() not in (1, 2):
                raise ValueError(f"{who}: labels must be an integer (N, A) array, one row per sample")
            labels = labels.reshape(labels.shape[0], -1)
            if labels.shape[0] != N or labels.shape[1] < 1:
                raise ValueError(f"{who}: labels is {tuple(labels.shape)}, the batches hold {N} rows (one ROW of label "
                                 f"columns per sample, in batch order)")
            if int(labels.min()) < 0:
                raise ValueError(f"{who}: labels holds negative values (classes are numbered from 0)")
            if not [k for k in ks if k <= keep]:
                raise ValueError(f"{who}: labels are read against the k <= keep nearest rows; ks = {ks}, keep = {keep}")
        scale = None
        if use == "posterior":
            with self._eval_noise():
                locs, scales, family = self._walk_posteriors(batches)
            if metric in ("w2", "skl"):
                for m in names:
                    if family[m] is not dist.Normal:
                        raise NotImplementedError(f"{who}: metric {metric!r} is the distance of diagonal Gaussians; the "
                                                  f"posterior of {m!r} is {family[m].__name__}")
                scale = torch.stack([scales[m] for m in names]).contiguous()
            loc = torch.stack([locs[m] for m in names]).contiguous()
        else:
            loc = torch.stack([torch.cat([self.latents_for(b, g) for b in batches]).float() for g in given]).contiguous()
        with torch.no_grad():
            got = ops.retrieval_ranks(loc, scale, metric=metric, keep=keep)
        less, equal = got["less"].cpu(), got["equal"].cpu()
        summary = ops.retrieval_summary(less, equal, ks=ks, n_gallery=N)
        nn_idx = got["nn_idx"].cpu()
        res = {}
        for p, (a, b) in enumerate(got["pairs"]):
            r = dict(summary[p])
            r.update(d_match=got["d_match"][p], rank=(1 + less[p] + equal[p]).to(torch.int32), nn_idx=got["nn_idx"][p])
            if labels is not None:
                r["label_precision"] = {c: ops.retrieval_label_precision(nn_idx[p], labels[:, c], labels[:, c],
                                                                         [k for k in ks if k <= keep])
                                        for c in range(labels.shape[1])}
            res[f"{keys[a]}->{keys[b]}"] = r
        res["mean"] = {k: sum(s[k] for s in summary) / len(summary) for k in summary[0]}
        return res

    # ---- reconstruction quality of generated images ---------------------------------------------------
    @staticmethod
    def _image_planes(data_dim):
        """the callable that lays a tensor of an image modality with this data_dim out as (rows, C, H, W), as the project
        reads that modality elsewhere, or None for a data_dim that is no known image form"""
        d = tuple(data_dim)
        if d in ((64, 64, 3), (3, 64, 64)):      # the CdSprites+ decoder labels its output by view and does not permute it
            return lambda t: t.reshape(-1, 3, 64, 64)      # (coherence.quantise_images)
        if d in ((28, 28, 1), (1, 28, 28)):
            return lambda t: t.reshape(-1, 1, 28, 28)
        if d in ((32, 32, 3), (3, 32, 32)):      # Dec_SVHN returns (.., 32, 32, 3): permuted back (DigitClassifier.images)
            return lambda t: (t.reshape(-1, 32, 32, 3).permute(0, 3, 1, 2) if tuple(t.shape[-3:]) == (32, 32, 3)
                              else t.reshape(-1, 3, 32, 32))
        return None

    def reconstruction_quality(self, batches, images=None, eps=None, **window):
        """How close a generated image is to the image it was generated for: PSNR, SSIM (Wang et al. 2004) and MS-SSIM, the
        mean squared and the mean absolute error, pair by pair in float64 on the device (ops.image_quality;
        csrc/image_quality.hip).  Row i of a reconstruction and of a cross-generation belongs to row i of the batch's data;
        joint samples have no partner and are not walked, so that the metric works for every mixer, private latents
        included.  `batches`: an iterable of batch dicts holding every modality.
        `images`: {modality: callable -> (rows, C, H, W)}, handed batch[m]["data"] for the real rows and decoder_dist.loc for
        generated ones (the first B rows are read).  The default takes every modality whose data_dim is a known image
        form, in the layout the project reads it in elsewhere: (64, 64, 3) -> reshape(-1, 3, 64, 64) (the CdSprites+ decoder's
        output is labelled, not permuted: coherence.quantise_images), (28, 28, 1) -> (-1, 1, 28, 28), (32, 32, 3) -> permuted
        back to (-1, 3, 32, 32) (DigitClassifier.images).
        `window`: win, sigma, data_range, k1, k2, sample_covariance, scales, weights of ops.image_quality.
        The sets and the order of the forward() calls are those of frechet_distances with n_joint = 0; each batch's real
        rows are kept as fp32 copies until the walk ends, every generated batch is scored as it arrives.
        -> {m: {"recon": {...}, "cross": {g: {...}}, "n": rows, "shape": (C, H, W),
                "per_sample": {"recon": {name: (n,)}, "cross": {g: {name: (n,)}}}}}, each {...} the float means over the rows of
        "psnr", "ssim", "ms_ssim", "mse", "mae" (psnr is +inf as soon as one row is reproduced exactly, as the per-image
        convention gives), per_sample the float64 tensors they are the means of and "levels" (n, scales).
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps`: a list of (B, D)
        tensors consumed in forward()'s draw order over all calls (as `eps_override`).  The training noise state, the
        dropout counters, gradients and the optimiser stay as they are."""
        who = "reconstruction_quality"
        self._need_eval(who, _GENERATIONS)
        names = list(self.vaes.keys())
        if images is None:
            images = {m: f for m, f in ((m, self._image_planes(self.vaes[m].data_dim)) for m in names) if f is not None}
            if not images:
                raise ValueError(f"{who}: no modality of this model has a known image form "
                                 f"({[tuple(self.vaes[m].data_dim) for m in names]}): name the layouts in `images`")
        elif not images or any(m not in names or not callable(f) for m, f in images.items()):
            raise ValueError(f"{who}: `images` maps modalities of this model ({names}) to callables")
        shapes, real, done, scores = {}, {}, {}, {}

        def flat(m):
            def planes(t):
                p = images[m](t)
                if not torch.is_tensor(p) or p.dim() != 4 or not p.is_floating_point():
                    raise ValueError(f"{who}: the callable of {m!r} must return float (rows, C, H, W) images")
                if shapes.setdefault(m, tuple(p.shape[1:])) != tuple(p.shape[1:]):
                    raise ValueError(f"{who}: the callable of {m!r} returned images of {tuple(p.shape[1:])} after "
                                     f"{shapes[m]}")
                return p.reshape(p.shape[0], -1)
            return planes

        def sink(m, key, f):
            if key == "real":
                ops.image_quality_plan((len(f),) + shapes[m], **window)      # (refusals before the first forward())
                real.setdefault(m, []).append(f.detach().to(torch.float32, copy=True))
                return
            b = done.get((m, key), 0)
            done[(m, key)] = b + 1
            x = real[m][b]
            if f.shape[0] != x.shape[0]:
                raise ValueError(f"{who}: {f.shape[0]} generated rows of {m!r} for the {x.shape[0]} rows of batch {b}")
            scores.setdefault((m, key), []).append(
                ops.image_quality(x.reshape(-1, *shapes[m]), f.detach().reshape(-1, *shapes[m]), **window))

        mods, _ = self._walk_generations(who, batches, {m: flat(m) for m in images}, 0, eps, None, lambda rows, n_joint: None,
                                         sink)
        stats = ("psnr", "ssim", "ms_ssim", "mse", "mae")
        res = {}
        with torch.no_grad():
            for m in mods:
                r = {"recon": None, "cross": {}, "n": sum(len(x) for x in real[m]), "shape": shapes[m],
                     "per_sample": {"recon": None, "cross": {}}}
                for (mm, key), parts in scores.items():
                    if mm != m:
                        continue
                    per = {name: torch.cat([p[name] for p in parts]) for name in stats + ("levels",)}
                    means = {name: float(per[name].mean()) for name in stats}
                    if isinstance(key, tuple):
                        r["cross"][key[1]], r["per_sample"]["cross"][key[1]] = means, per
                    else:
                        r[key], r["per_sample"][key] = means, per
                res[m] = r
        return res

    # ---- text generation quality ---------------------------------------------------------------------
    def text_quality(self, batches, texts=None, eps=None, eos=None, trim=0, sep=0, max_order=4):
        """How close a generated caption is to the caption it was generated for: character and word error rate (Levenshtein
        distance), BLEU, ROUGE-L, exact match and position accuracy of the decoder's argmax string, and the perplexity of
        the true tokens under the decoder's logits, pair by pair on the device (ops.text_quality; csrc/text_quality.hip).
        Row i of a reconstruction and of a cross-generation belongs to row i of the batch's data; joint samples have no
        partner and are not walked, so that the metric works for every mixer.  `batches`: an iterable of batch dicts holding
        every modality, the text ones one-hot (B, T, V); the references are read from the batches themselves as
        cross_coherence reads them (argmax of the one-hot rows, the length from the mask, T where masks are None).
        `texts`: the modalities to score; the default takes every modality with a Dec_TxtTransformer decoder and a data_dim
        (T, V, 1) inside the kernel's limits.  `eos`, `trim`, `sep`, `max_order`: as ops.text_quality; the defaults trim = 0,
        sep = 0 are the convention of the CdSprites+ and CUB captions here (id 0 is the space, padding decodes to 0).
        The sets and the order of the forward() calls are those of reconstruction_quality: per batch the full batch, then only
        modality g given for every g that a scored modality is generated from, in modality order.  A text modality that is
        not given to a call decodes at full length (its masks are None for that call, as in cross_coherence); where it is
        given -- the reconstruction -- its masks stay, since its encoder reads them, and the decoder's zero rows at the
        padded steps decode to id 0.  So the "recon" figures mean what they say only while `trim` is that padding id, 0
        (the default): with trim None or another id, every masked reconstruction carries its T - length trailing zeros
        into the edit distance, the n-gram totals and, through sep, the word counts; the "cross" figures do not depend on it.
        Of a generation's rows the first B are scored (the first component of a mixer that decodes several).
        -> {m: {"recon": S, "cross": {g: S}, "n": rows, "per_sample": {"recon": P, "cross": {g: P}}}}, S the
        ops.text_quality_summary dict {"token": {...}, "word": {...}}, P the ops.text_quality dict of the concatenated
        per-pair device tensors (`pred` padded with -1 to the longest decoding).
        Needs eval mode; runs without gradients; noise from the evaluation generator, or from `eps`: a list of (B, D)
        tensors consumed in forward()'s draw order over all calls (as `eps_override`).  The training noise state, the
        dropout counters, gradients and the optimiser stay as they are."""
        who = "text_quality"
        self._need_eval(who, _GENERATIONS)
        names, batches = list(self.vaes.keys()), list(batches)
        if not batches:
            raise ValueError(f"{who}: `batches` is empty")
        dims = {m: tuple(self.vaes[m].data_dim) for m in names}
        if texts is None:
            texts = [m for m in names if isinstance(self.vaes[m].dec, Dec_TxtTransformer) and len(dims[m]) == 3
                     and dims[m][2] == 1 and 1 <= dims[m][0] <= ops.H.TQ_MAX_STEPS and 2 <= dims[m][1] <= ops.H.TQ_MAX_VOCAB]
            if not texts:
                raise ValueError(f"{who}: no modality of this model is a text tower (a Dec_TxtTransformer with data_dim (T, V, 1), "
                                 f"T <= {ops.H.TQ_MAX_STEPS}, V <= {ops.H.TQ_MAX_VOCAB}; the data dims are "
                                 f"{[dims[m] for m in names]}): name them in `texts`")
        else:
            texts = [texts] if isinstance(texts, str) else list(texts)
            if not texts or len(set(texts)) != len(texts) or any(m not in names for m in texts):
                raise ValueError(f"{who}: `texts` lists modalities of this model ({names})")
        texts = [m for m in names if m in texts]
        refs = {m: [] for m in texts}
        for batch in batches:
            if any(m not in batch or batch[m]["data"] is None for m in names):
                raise ValueError(f"{who}: every batch must hold every modality (a modality without data)")
            for m in texts:
                onehot, masks = batch[m]["data"], batch[m]["masks"]
                if onehot.dim() != 3 or not onehot.is_floating_point():
                    raise ValueError(f"{who}: the text modality {m!r} must be one-hot (B, T, V), got {tuple(onehot.shape)}")
                B, T, V = onehot.shape
                ops.text_quality_plan(dims[m][0], T, V, eos, trim, sep, max_order)      # (refusals before the first forward())
                if masks is not None and tuple(masks.reshape(B, -1).shape) != (B, T):
                    raise ValueError(f"{who}: the masks of {m!r} are {tuple(masks.shape)} for data {tuple(onehot.shape)}")
                refs[m].append((B, onehot, masks))
        scores = {}

        def score(m, key, b, loc):
            B, V, ids, lens = refs[m][b]
            if loc.dim() < 3 or loc.shape[-1] != V:
                raise ValueError(f"{who}: the decoder of {m!r} returned {tuple(loc.shape)}; logits (rows, T, {V})")
            logits = loc.reshape(-1, *loc.shape[-2:])
            if logits.shape[0] < B:
                raise ValueError(f"{who}: {logits.shape[0]} generated rows of {m!r} for the {B} rows of batch {b}")
            scores.setdefault((m, key), []).append(
                ops.text_quality(logits[:B].detach(), ids, lens, None, eos=eos, trim=trim, sep=sep, max_order=max_order))

        with self._eval_noise(eps):
            for m in texts:
                for b, (B, onehot, masks) in enumerate(refs[m]):
                    ids, _ = ops.text_decode_score(onehot.float().contiguous())
                    lens = (torch.full((B,), onehot.shape[1], dtype=torch.int32, device=onehot.device) if masks is None
                            else torch.count_nonzero(masks.reshape(B, -1), dim=-1).to(torch.int32))
                    refs[m][b] = (B, onehot.shape[2], ids, lens)
            for b, batch in enumerate(batches):
                out = self.forward(batch)
                for m in texts:
                    score(m, "recon", b, out.mods[m].decoder_dist.loc)
                for g in names:
                    if any(m != g for m in texts):
                        x = self._given_only(batch, [g])
                        for m in texts:
                            if m != g:
                                x[m] = dict(x[m], masks=None)
                        out = self.forward(x)
                        for m in texts:
                            if m != g:
                                score(m, ("cross", g), b, out.mods[m].decoder_dist.loc)
            res = {}
            for m in texts:
                r = {"recon": None, "cross": {}, "n": sum(ref[0] for ref in refs[m]), "per_sample": {"recon": None, "cross": {}}}
                for (mm, key), parts in scores.items():
                    if mm != m:
                        continue
                    S, P = ops.text_quality_summary(parts), self._cat_text_quality(parts)
                    if isinstance(key, tuple):
                        r["cross"][key[1]], r["per_sample"]["cross"][key[1]] = S, P
                    else:
                        r[key], r["per_sample"][key] = S, P
                res[m] = r
        return res

    @staticmethod
    def _cat_text_quality(parts):
        """the ops.text_quality dicts of several batches as one (`pred` padded with -1 to the longest decoding)"""
        level = lambda name: (None if parts[0][name] is None
                              else {k: torch.cat([p[name][k] for p in parts]) for k in parts[0][name]})
        Th = max(p["pred"].shape[1] for p in parts)
        pred = torch.cat([torch.nn.functional.pad(p["pred"], (0, Th - p["pred"].shape[1]), value=-1) for p in parts])
        return {"token": level("token"), "word": level("word"), "pred": pred, "nll": torch.cat([p["nll"] for p in parts]),
                "nll_steps": torch.cat([p["nll_steps"] for p in parts]), "max_order": parts[0]["max_order"]}
