#!/usr/bin/env python3
"""Link prediction with an R-GCN encoder + DistMult decoder on MI355X -- counterpart of the reference's
experiments/predict_links.py (:19-228) without sacred.  Reads the reference's config schema unchanged:

    python experiments/predict_links.py configs/rgcn/lp-WN18.yaml [--data DIR] [--epochs N]

training.{epochs,graph_batch_size,sampling_method,negative_sampling.{sampling_rate,head_prob},optimiser.*}
training.objective (an extension, absent in the reference): "negative-sampling" (default: the reference's sampled-negative BCE) or "1-n"
(softmax cross-entropy of every sampled positive against ALL entities, tails and heads; configs/rgcn/lp-WN18-1n.yaml);
training.filtered (1-n only, default false; configs/rgcn/lp-WN18-1n-filtered.yaml): the other known completions of a query -- from the
TRAINING triples only -- are left out of its softmax, looked up in a device-resident FilterIndex, so the step is captured all the same
training.bf16 (1-n only, default false; configs/rgcn/lp-WN18-1n-bf16.yaml): the model is put into bf16 (model.bfloat16()) before the
optimiser is built and both softmax terms run the native bf16 backward -- no fp32 image of the entity table exists during training
training.label_smoothing (1-n only, default 0; configs/rgcn/lp-WN18-1n-smoothed.yaml): epsilon in [0, 1) of both softmax terms, spread
evenly over the candidates that are not filtered; combines with training.filtered and training.bf16, and the step is captured all the same
training.objective "1-n-bce" (configs/rgcn/lp-WN18-1n-bce.yaml): the K-vs-All binary cross-entropy -- every sampled positive against ALL
entities, tails and heads, every known completion of a query among the TRAINING triples a positive label and everything else a negative;
the labels come from a device-resident FilterIndex, built once and always on (that is what K-vs-All means), so training.filtered with it
raises ValueError; training.bf16 and training.label_smoothing (here eps / N over all entities) combine with it, the step is captured
decoder.model (the reference's schema carries the key and never reads it): "complex" builds the ComplEx decoder (an extension;
configs/rgcn/lp-WN18-complex.yaml, lp-WN18-1n-complex.yaml) -- an even node_embedding read as real halves | imaginary halves -- for every
objective above, evaluation and prediction included; any other value, or none, is DistMult
encoder.{model,...,edge_dropout.general}  decoder.l2_penalty  evaluation.{final_run,filtered,check_every,batch_size,verbose}.
Differences: the positives are sampled by the native edge-neighbourhood sampler (milliseconds instead of minutes per
epoch), negatives are drawn on the GPU, and evaluation encodes the training graph once (utils/misc.py)."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_rgcn  # noqa: E402
from torch_rgcn import routes  # noqa: E402
from torch_rgcn.functional import FilterIndex, bce_with_logits, unit_gradient  # noqa: E402
from torch_rgcn.models import CompressionRelationPredictor, LinkPredictor  # noqa: E402
from utils.data import load_link_prediction_data  # noqa: E402
from utils.misc import evaluate, generate_true_dict, negative_sampling, select_sampling  # noqa: E402

OPTIMISERS = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "adagrad": torch.optim.Adagrad, "sgd": torch.optim.SGD}


def step_loss(model, graph, batch_idx, train_lbl, objective="negative-sampling", train_filter=None, loss_kw=None, decoder_l2_penalty=0.0):
    """The scalar loss of one training step of `model` (LinkPredictor / CompressionRelationPredictor) on the message graph `graph`.
    objective "negative-sampling": batch_idx holds the positives and their corrupted copies, train_lbl their 1 / 0 labels -- the mean BCE.
    "1-n" / "1-n-bce": batch_idx holds the positives alone (train_lbl is not read) -- half the tail loss plus half the head loss over ALL
    entities; train_filter: the FilterIndex of the cells left out (1-n; None: unfiltered) or of the positive labels (1-n-bce);
    loss_kw: bf16_backward / label_smoothing of both terms.  decoder_l2_penalty times model.compute_penalty is added in every objective."""
    if objective not in ("negative-sampling", "1-n", "1-n-bce"):
        raise NotImplementedError(f"'{objective}' training objective has not been implemented!")
    if objective in ("1-n", "1-n-bce"):   # half the tail loss, half the head loss (static shapes, filtered or not: the captured step works)
        x = model.encode(graph)
        decoder_ = model.scoring_function
        loss_kw = loss_kw or {}
        if objective == "1-n-bce":        # the index holds the positive labels
            term = lambda head: decoder_.bce_loss(batch_idx, x, head=head, labels=train_filter, **loss_kw)  # noqa: E731
        else:                             # the index (if any) holds the cells left out
            term = lambda head: decoder_.softmax_loss(batch_idx, x, head=head, filt=train_filter, **loss_kw)  # noqa: E731
        loss = 0.5 * (term(False) + term(True))
        return loss + decoder_l2_penalty * model.compute_penalty(batch_idx, x)
    predictions, penalty = model(graph, batch_idx)
    return bce_with_logits(predictions, train_lbl) + decoder_l2_penalty * penalty


def run(cfg, data_dir=None, epochs=None, quiet=False, max_test=None, synthetic=None, hipgraph=None, fused_eval=None, device_filter=False):
    """-> (loss per epoch, {"mrr", "hits@1", "hits@3", "hits@10"} of the final evaluation).
    The training step (per-step graph build, encoder, decoder, loss, backward, optimiser) is captured once in a hipGraph and replayed
    every epoch on freshly sampled inputs copied into static buffers -- BY DEFAULT (hipgraph=None: unless route `capture` is "0";
    falls back to the eager loop, with a warning, if the capture fails; True insists, False is the reference's loop literally).
    The capture runs under the sync-free plan builder (route deferred_checks = 1, scoped to the warm-up and the capture).
    fused_eval: utils.misc.evaluate's `fused` (True: rank without the score matrix; None: only where that matrix would need chunks).
    device_filter: utils.misc.evaluate's `device_filter` (the evaluation filter from a device-resident index, no host lists)."""
    dataset, training, encoder = cfg["dataset"], cfg["training"], cfg["encoder"]
    decoder, evaluation = cfg.get("decoder", {}), cfg.get("evaluation", {})
    objective = training.get("objective", "negative-sampling")
    if objective not in ("negative-sampling", "1-n", "1-n-bce"):
        raise NotImplementedError(f"'{objective}' training objective has not been implemented!")
    k_vs_all = objective == "1-n-bce"
    one_to_n = objective == "1-n" or k_vs_all          # every entity is a candidate of every positive
    train_filtered = bool(training.get("filtered", False))
    if train_filtered and k_vs_all:
        raise ValueError("training.filtered does not combine with training.objective: 1-n-bce (the known completions are its positive labels)")
    if train_filtered and not one_to_n:
        raise ValueError("training.filtered needs training.objective: 1-n (sampled negatives are not filtered)")
    train_bf16 = bool(training.get("bf16", False))
    if train_bf16 and not one_to_n:
        raise ValueError("training.bf16 needs training.objective: 1-n or 1-n-bce (the native bf16 backward is the 1-N losses')")
    label_smoothing = training.get("label_smoothing", 0)
    if label_smoothing and not one_to_n:
        raise ValueError("training.label_smoothing needs training.objective: 1-n or 1-n-bce (the sampled-negative objective has no smoothing)")
    max_epochs = epochs or training.get("epochs", 5000)
    graph_batch_size = training.get("graph_batch_size")
    sampling_function = select_sampling(training.get("sampling_method", "uniform"))
    neg_sample_rate = training.get("negative_sampling", {}).get("sampling_rate")
    head_corrupt_prob = training.get("negative_sampling", {}).get("head_prob")
    edge_dropout = encoder.get("edge_dropout", {}).get("general", 0.0) if encoder.get("edge_dropout") else 0.0
    decoder_l2_penalty = decoder.get("l2_penalty", 0.0)
    filtered = evaluation.get("filtered", False)
    eval_every = evaluation.get("check_every", 2000)
    eval_kw = dict(batch_size=evaluation.get("batch_size", 16), verbose=evaluation.get("verbose", False) and not quiet,
                   filter_candidates=filtered, fused=fused_eval, device_filter=device_filter)

    (n2i, nodes), (r2i, relations), train, test, all_triples = load_link_prediction_data(
        dataset["name"], use_test_set=evaluation.get("final_run", False), directory=data_dir, synthetic=synthetic)
    true_triples = generate_true_dict(all_triples)
    if max_test:
        test = test[:max_test]

    # block decomposition: pad the node list to a multiple of the block size (predict_links.py:54-67)
    if encoder.get("decomposition") and encoder["decomposition"]["type"] == "block":
        if "node_embedding" not in encoder:
            raise ValueError()
        block_size = encoder["node_embedding"] / encoder["decomposition"]["num_blocks"]
        added = 0
        while len(nodes) % block_size != 0:
            label = "null" + str(added)
            nodes.append(label)
            n2i[label] = len(nodes) - 1
            added += 1
        if not quiet:
            print(f"nodes padded to {len(nodes)} to make it divisible by {block_size} (added {added} null nodes).")

    device = torch.device("cuda")
    num_nodes, num_relations = len(n2i), len(r2i)
    test = torch.tensor(test, dtype=torch.long)
    train = np.asarray(train, dtype=np.int64)          # sampled from every epoch: keep it an array
    train_graph = torch.from_numpy(train)
    # the filter of the 1-N loss: the TRAINING triples alone (validation and test triples must not reach the loss), indexed once
    # (1-n-bce: the same index holds the positive labels, always)
    train_filter = FilterIndex(generate_true_dict(train), num_nodes, device) if train_filtered or k_vs_all else None
    if encoder["model"] == "rgcn":
        kind = LinkPredictor
    elif encoder["model"] == "c-rgcn":
        kind = CompressionRelationPredictor
    else:
        raise NotImplementedError(f"'{encoder['model']}' encoder has not been implemented!")
    model = kind(nnodes=num_nodes, nrel=num_relations, encoder_config=encoder, decoder_config=decoder).to(device)
    if train_bf16:
        model = model.bfloat16()
    loss_kw = {"bf16_backward": "native"} if train_bf16 else {}
    if label_smoothing:
        loss_kw["label_smoothing"] = label_smoothing
    opt_cfg = training.get("optimiser", {"algorithm": "adam", "learn_rate": 0.01, "weight_decay": 0.0})
    if opt_cfg["algorithm"] not in OPTIMISERS:
        raise NotImplementedError(f"'{opt_cfg['algorithm']}' optimiser has not been implemented!")
    extra = {"fused": True} if opt_cfg["algorithm"] in ("adam", "adamw") else {}
    insist = hipgraph is True
    if insist and not torch_rgcn.REPLAY_SAFE:
        import warnings
        warnings.warn("hipgraph=True although DEBUG_CLR_GRAPH_PACKET_CAPTURE was not 0 when the HIP runtime started: replays of a captured "
                      "step are known to go wrong on this runtime (torch_rgcn/__init__.py)")
    if hipgraph is None:
        hipgraph = routes.get("capture", "1") != "0" and torch_rgcn.REPLAY_SAFE
    if hipgraph:
        # a captured step cannot read the device-side range-check flags back: validate the triples the sampler draws from HERE,
        # once, on the host (the kernels additionally clamp and kill out-of-range triples, csrc/rgcn_build.hip)
        tr = np.asarray(train)
        assert tr.size == 0 or (tr[:, [0, 2]].min() >= 0 and tr[:, [0, 2]].max() < num_nodes and tr[:, 1].min() >= 0
                                and tr[:, 1].max() < num_relations), "training triples: node or relation index out of range"
        extra = {"capturable": True} if opt_cfg["algorithm"] in ("adam", "adamw") else {}
    optimiser = OPTIMISERS[opt_cfg["algorithm"]](model.parameters(), lr=opt_cfg["learn_rate"],
                                                  weight_decay=opt_cfg["weight_decay"], **extra)

    def report(tag, mrr, hits):
        kind_ = "filtered" if filtered else "raw"
        print(f"{tag} MRR({kind_}): {mrr:.4f} \tHits@1({kind_}): {hits[0]:.4f} \tHits@3({kind_}): {hits[1]:.4f} \t"
              f"Hits@10({kind_}): {hits[2]:.4f}")

    def sample_inputs():
        """one epoch's positives / negatives / labels / message graph (all sizes are the same every epoch)"""
        nonlocal graph_batch_size
        with torch.no_grad():
            if graph_batch_size is None:          # the whole graph
                positives, graph_batch_size = train, len(train)
            else:
                positives = sampling_function(train, sample_size=graph_batch_size, entities=n2i)
            positives = torch.as_tensor(positives, dtype=torch.long).to(device)
            if one_to_n:                          # every entity is a candidate: nothing to draw, no labels
                batch_idx, train_lbl = positives, torch.empty(0, device=device)
            else:
                batch_idx, train_lbl = corrupt(positives)
            graph = positives
            if edge_dropout > 0.0:                # self-loop dropout happens inside the layer
                graph = graph[torch.randperm(graph.size(0), device=device)]
                graph = graph[round((1 - edge_dropout) * graph.size(0)):, :]     # (keeps the edge_dropout share, as upstream)
        return graph, batch_idx, train_lbl

    def corrupt(positives):
        """the reference's batch: the positives, then neg_sample_rate corrupted copies of each, and their labels"""
        negatives = positives[:, None, :].expand(graph_batch_size, neg_sample_rate, 3).contiguous()
        negatives = negative_sampling(negatives, num_nodes, head_corrupt_prob, device=device)
        batch_idx = torch.cat([positives, negatives], dim=0)
        train_lbl = torch.cat([torch.ones(graph_batch_size, device=device),
                               torch.zeros(graph_batch_size * neg_sample_rate, device=device)])
        return batch_idx, train_lbl

    def train_step(graph, batch_idx, train_lbl):
        optimiser.zero_grad(set_to_none=False)
        loss = step_loss(model, graph, batch_idx, train_lbl, objective, train_filter, loss_kw, decoder_l2_penalty)
        loss.backward(gradient=unit_gradient(loss.device))      # (no ones_like() fill per step; MaskedCrossEntropy skips the multiplication)
        optimiser.step()
        return loss

    captured = None
    if hipgraph:
        model.train()
        # the step is captured once on static input buffers; every epoch samples as the eager loop does (on the GPU) and copies
        # into them.  (Round 2 history: replays used to fault whenever eager kernels ran between them -- the HIP runtime replays
        # hipMemsetAsync NODES with stale arguments; the library zero-fills with kernels now, tools/hipgraph_repro/.)
        static = [t.clone() for t in sample_inputs()]
        # the warm-up steps below are real optimiser steps: parameters and optimiser state are put back afterwards (in place -- the
        # captured graph holds their addresses), so that a captured run starts epoch 1 from the same state as the eager run
        saved_params = [p.detach().clone() for p in model.parameters()]
        try:
            with routes.override(deferred_checks="1"):       # no device -> host reads inside the captured step
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                    # warm-up off the capture: allocator pools, lazy inits
                    for _ in range(3):
                        train_step(*static)
                torch.cuda.current_stream().wait_stream(side)
                captured = torch.cuda.CUDAGraph()
                with torch.cuda.graph(captured):
                    static_loss = train_step(*static)
        except Exception as exc:  # noqa: BLE001  (the eager loop runs the same HIP kernels: a slower path, not another implementation)
            if insist:
                raise
            import warnings
            warnings.warn(f"hipGraph capture of the training step failed ({type(exc).__name__}: {exc}); running the eager loop")
            torch.cuda.synchronize()
            captured = None
        with torch.no_grad():
            for p, q in zip(model.parameters(), saved_params):
                p.copy_(q)
            for st in optimiser.state.values():              # Adam / SGD-momentum state after zero steps: all zeros
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
        del saved_params

    losses = []
    for epoch in range(1, max_epochs + 1):
        t1 = time.time()
        model.train()
        if captured is not None:
            for buf, fresh in zip(static, sample_inputs()):
                buf.copy_(fresh)
            captured.replay()
            loss = static_loss
            t2 = time.time()
        else:
            optimiser.zero_grad()
            graph, batch_idx, train_lbl = sample_inputs()
            loss = step_loss(model, graph, batch_idx, train_lbl, objective, train_filter, loss_kw, decoder_l2_penalty)
            t2 = time.time()
            loss.backward(gradient=unit_gradient(loss.device))
            optimiser.step()
        torch.cuda.synchronize()
        t3 = time.time()
        losses.append(loss.item())
        if not quiet:
            print(f"[Epoch {epoch}] Loss: {loss.item():.5f} Forward: {t2 - t1:.3f}s Backward: {t3 - t2:.3f}s ")
        if epoch % eval_every == 0 and epoch != max_epochs:
            model.eval()
            mrr, hits, _ = evaluate(model=model, graph=train_graph, test_set=test, true_triples=true_triples,
                                    num_nodes=num_nodes, **eval_kw)
            if not quiet:
                report(f"[Epoch {epoch}]", mrr, hits)

    model.eval()
    t0 = time.time()
    mrr, hits, ranks = evaluate(model=model, graph=train_graph, test_set=test, true_triples=true_triples,
                                num_nodes=num_nodes, **eval_kw)
    if not quiet:
        report(f"[Final Scores] Total Epoch {max_epochs} ({len(test)} test triples ranked in {time.time() - t0:.2f}s)", mrr, hits)
    return losses, {"mrr": mrr, "hits@1": hits[0], "hits@3": hits[1], "hits@10": hits[2]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--data", default=None, help="directory holding data/<name>/{train,valid,test}.txt")
    ap.add_argument("--synthetic", action="store_true", help="when the dataset files are absent, train on a random graph with "
                    "the dataset's entity / relation / triple counts (timing and plumbing only: MRR / Hits mean nothing)")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--max-test", type=int, default=None)
    ap.add_argument("--hipgraph", action="store_true", help="insist on the captured training step (the default tries it and falls back to eager)")
    ap.add_argument("--eager", action="store_true", help="the reference's loop literally: no hipGraph capture")
    ap.add_argument("--fused-eval", action="store_true", help="rank with the fused evaluator (no score matrix) whatever the size; "
                    "the default takes it only where the score matrix of the test set exceeds the 1 GiB chunk budget")
    ap.add_argument("--device-filter", action="store_true", help="evaluate with the filter looked up in a device-resident index "
                    "instead of host-built lists per chunk (the same ranks)")
    a = ap.parse_args()
    run(yaml.safe_load(open(a.config)), a.data, a.epochs, max_test=a.max_test, synthetic=True if a.synthetic else None,
        hipgraph=False if a.eager else (True if a.hipgraph else None), fused_eval=True if a.fused_eval else None,
        device_filter=a.device_filter)
