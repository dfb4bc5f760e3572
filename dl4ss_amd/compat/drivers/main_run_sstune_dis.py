"""py3 mirror of ``TDAA_beta/main_run_sstune_dis.py`` -- the separation net of the sstune drivers
(BiGRU MIX_SPEECH, 'dot' attention, ADDJUST) trained against the adversarial ``Discriminator``
(LSGAN-style: MSE of the sigmoid score against 1 / 0), Adam 2e-4 with the 10-epoch LR halving.

It imports the reference driver's module names (``config_WSJ0_dB as config``,
``test_multi_labels_speech``, ``bss_test``, ``lrs``, ``librosa``, ``soundfile``;
``compat.install()`` resolves them), defines the driver's module variants over ``myNet`` (every
forward / backward on the HIP kernels, the Discriminator's convolutions included) and runs the
reference's loop (``main`` :486-665).  Differences from the reference, each deliberate:

* one forward, two gradient sets, then the two updates.  The reference calls
  ``loss_dis.backward(retain_graph=True); optimizer.step()`` and then walks the retained graph again
  with ``loss_multi_speech.backward()`` (:626-628, :645-647) -- after the first step changed, in
  place, weights that graph saved.  torch 0.3 did not version-check saved tensors; today's torch
  refuses the second backward.  Here both gradient sets are taken from the one forward BEFORE either
  update (``torch.autograd.grad(..., retain_graph=True, allow_unused=True)``), then the two Adam
  steps are applied in the reference's order.  The second update therefore uses gradients at the
  pre-step weights, where torch 0.3 mixed pre- and post-step weights inside one backward;
* the fake maps are not detached in the reference's Discriminator loss (:616,623), so its first step
  also moves every separation parameter ``loss_dis`` reaches.  That is kept as the default
  (``detach_fake=False``); ``detach_fake=True`` gives the textbook update, in which the first step
  touches the Discriminator alone;
* the loader is ``predata_fromList`` (the C2 list loader): ``predata_fromList_dis`` differs from it by
  ``sample_from_spk``, which needs the WSJ0 speaker directories.  ``train_step(..., y_true_map=...)``
  takes the other-utterance true maps of ``main_run_sstune_dis_sp.py:613-624`` from a caller that has
  them;
* ``torch.optim.Adam`` is the HIP Adam of ``compat.optim`` (same param_groups interface);
* the reference's ``Linear(36480, 1)`` is sized from (mix_speech_len, speech_fre) (36480 at (313, 129));
* the per-epoch ``eval_bss`` (:663-665) is not part of the training step and is left out.
"""
import os
import random

import numpy as np
import torch

try:
    from dl4ss_amd import compat as _compat
except ImportError:  # pragma: no cover
    _compat = None
if _compat is not None:
    _compat.install()

import config_WSJ0_dB as config  # noqa: E402
from predata_fromList import prepare_data, prepare_datasize  # noqa: E402,F401
from test_multi_labels_speech import multi_label_vector  # noqa: E402
import bss_test  # noqa: E402,F401
import lrs  # noqa: E402
import librosa  # noqa: E402,F401
import soundfile as sf  # noqa: E402,F401
import myNet  # noqa: E402

from dl4ss_amd.compat.optim import Adam  # noqa: E402
from dl4ss_amd.compat.drivers import _common as C  # noqa: E402
from dl4ss_amd import checkpoint, schedule  # noqa: E402

test_all_outputchannel = 0


class MIX_SPEECH(myNet.MIX_SPEECH):
    """dis.py:268-293: nn.GRU(input_fre, HIDDEN_UNITS, NUM_LAYERS) + Linear + tanh, returns (V, h)."""

    def __init__(self, input_fre, mix_speech_len):
        super().__init__(input_fre, mix_speech_len, cell="gru", num_layers=config.NUM_LAYERS, return_hidden=True,
                         precision=getattr(config, "PRECISION", "fp32"))


class MIX_SPEECH_classifier(myNet.MIX_SPEECH_classifier):
    """dis.py:295-316: BiLSTM with hidden 2 HIDDEN_UNITS, NUM_LAYERS layers, mean over t, sigmoid."""

    def __init__(self, input_fre, mix_speech_len, num_labels):
        super().__init__(input_fre, mix_speech_len, num_labels, hidden=2 * config.HIDDEN_UNITS,
                         num_layers=config.NUM_LAYERS, precision=getattr(config, "PRECISION", "fp32"))


class Discriminator(myNet.Discriminator):
    """dis.py:318-336, sized from the map instead of the constant 36480."""

    def __init__(self, mix_speech_len=313, speech_fre=129):
        super().__init__(mix_speech_len, speech_fre, precision=getattr(config, "PRECISION", "fp32"))


class SPEECH_EMBEDDING(myNet.SPEECH_EMBEDDING):
    """dis.py:338-351 (the gather form, width EMBEDDING_SIZE)."""

    def __init__(self, num_labels, embedding_size, max_num_channel):
        super().__init__(num_labels, embedding_size, max_num_channel, crm=False)


class ADDJUST(myNet.ADDJUST):
    """dis.py:353-367."""

    def __init__(self, hidden_units, embedding_size):
        super().__init__(hidden_units, embedding_size, crm=False)


class ATTENTION(myNet.ATTENTION):
    """dis.py:190-234 ('dot')."""

    def __init__(self, hidden_size, mode='dot'):
        super().__init__(hidden_size, mode, crm=False)


top_k_mask = myNet.top_k_mask


def build(speech_fre, mix_speech_len, num_labels, spk_num_total, lr_data=0.0002):
    """dis.py:500-521: modules on the GPU + one Adam over six groups, the Discriminator the sixth."""
    d = C.dev()
    m = dict(mix_hidden_layer_3d=MIX_SPEECH(speech_fre, mix_speech_len).to(d),
             mix_speech_classifier=MIX_SPEECH_classifier(speech_fre, mix_speech_len, num_labels).to(d),
             mix_speech_multiEmbedding=SPEECH_EMBEDDING(num_labels, config.EMBEDDING_SIZE,
                                                        spk_num_total + config.UNK_SPK_SUPP).to(d),
             att_speech_layer=ATTENTION(config.EMBEDDING_SIZE, 'dot').to(d),
             adjust_layer=ADDJUST(2 * config.HIDDEN_UNITS, config.EMBEDDING_SIZE).to(d),
             dis_layer=Discriminator(mix_speech_len, speech_fre).to(d))
    optimizer = Adam([{'params': m['mix_hidden_layer_3d'].parameters()},
                      {'params': m['mix_speech_multiEmbedding'].parameters()},
                      {'params': m['mix_speech_classifier'].parameters()},
                      {'params': m['adjust_layer'].parameters()},
                      {'params': m['att_speech_layer'].parameters()},
                      {'params': m['dis_layer'].parameters()}], lr=lr_data)
    return m, optimizer


def _apply(optimizer, params, grads):
    """``optimizer.zero_grad(); <grads>; optimizer.step()`` with the gradients given."""
    optimizer.zero_grad()
    for p, g in zip(params, grads):
        p.grad = g
    optimizer.step()


def train_step(m, optimizer, train_data, dict_spk2idx, dict_idx2spk, num_labels, run_classifier=True,
               detach_fake=False, y_true_map=None):
    """One pass of dis.py:559-647 on a batch dict.  ``y_true_map`` (B, K, T, F): true maps shown to the
    Discriminator instead of the batch's own targets (dis_sp.py:613-624).  Returns a dict with the loss
    terms, the scores, the masks, the masked prediction and the true maps, and -- taken before either
    update -- the Discriminator's gradients of ``loss_dis`` (``dis_grads``, by parameter name) and the
    adversarial term's gradient at the prediction (``dpred_adv``)."""
    x = C.cuda(train_data['mix_feas'])
    B, T, F = x.shape
    mix_speech_hidden, mix_tmp_hidden = m['mix_hidden_layer_3d'](x)
    if run_classifier:  # :564, computed and then replaced by the ground truth (:570-571)
        with torch.no_grad():
            m['mix_speech_classifier'](x)
    top_k_mask_mixspeech, top_k_mask_idx, _ = C.ground_truth_selection(
        train_data, dict_spk2idx, num_labels, multi_label_vector, top_k_mask)
    mix_speech_multiEmbs = m['mix_speech_multiEmbedding'](top_k_mask_mixspeech, top_k_mask_idx)
    mix_adjust = m['adjust_layer'](mix_tmp_hidden, mix_speech_multiEmbs)
    mix_speech_multiEmbs = mix_adjust + mix_speech_multiEmbs
    assert len(top_k_mask_idx[0]) == len(top_k_mask_idx[-1])
    top_k_num = len(top_k_mask_idx[0])
    multi_mask = C.expanded_attention(m['att_speech_layer'], mix_speech_hidden, mix_speech_multiEmbs, B, top_k_num,
                                      T, F, config.EMBEDDING_SIZE)
    y_multi_map = C.label_ordered_targets(train_data, top_k_mask_idx, dict_spk2idx, dict_idx2spk,
                                          (B, top_k_num, T, F))
    # :602-613,631-638: MSE(mask * |X|, Y) + 0.5 MSE(sum_k mask, 1)
    loss_sep, predict_multi_map, l_mask, l_sum = C.magnitude_loss(multi_mask, x, y_multi_map)

    dis_layer = m['dis_layer']
    y_true = y_multi_map if y_true_map is None else C.cuda(np.asarray(y_true_map, dtype=np.float32))
    ones = torch.ones(B * top_k_num, 1, device=x.device)
    zeros = torch.zeros(B * top_k_num, 1, device=x.device)
    score_true = dis_layer(y_true)                    # :615
    score_false = dis_layer(predict_multi_map)        # :616
    score_false_dis = dis_layer(predict_multi_map.detach()) if detach_fake else score_false
    acc_true = float((score_true > 0.5).sum()) / score_true.shape[0]     # :617-619
    acc_false = float((score_false < 0.5).sum()) / score_true.shape[0]
    loss_dis_true = C.MSE(score_true, ones)           # :622-624
    loss_dis_false = C.MSE(score_false_dis, zeros)
    loss_dis = loss_dis_true + loss_dis_false
    loss_adv = C.MSE(score_false, ones)               # :642-643
    loss = loss_sep + loss_adv
    lrs.send('loss mask:', float(l_mask))
    lrs.send('loss sum:', float(l_sum))

    params = [p for g in optimizer.param_groups for p in g['params']]
    g_dis = torch.autograd.grad(loss_dis, params, retain_graph=True, allow_unused=True)
    (dpred_adv,) = torch.autograd.grad(loss_adv, predict_multi_map, retain_graph=True)
    g_sep = torch.autograd.grad(loss, params, allow_unused=True)
    by_param = {id(p): g for p, g in zip(params, g_dis)}
    dis_grads = {n: by_param[id(p)].detach().clone() for n, p in dis_layer.named_parameters()}
    _apply(optimizer, params, g_dis)   # :626-628
    _apply(optimizer, params, g_sep)   # :645-647
    return dict(loss=loss.detach(), loss_dis=loss_dis.detach(), loss_dis_true=loss_dis_true.detach(),
                loss_dis_false=loss_dis_false.detach(), loss_adv=loss_adv.detach(), loss_mask=l_mask.detach(),
                loss_sum=l_sum.detach(), acc_dis=(acc_true + acc_false) / 2, score_true=score_true.detach(),
                score_false=score_false.detach(), mask=multi_mask.detach(), pred=predict_multi_map.detach(),
                y_true=y_true.detach(), dis_grads=dis_grads, dpred_adv=dpred_adv.detach(),
                top_k_mask_idx=top_k_mask_idx)


def save_params(m, epoch_idx, directory="params"):
    """dis.py:653-662: the five per-module files ``param_mix{mode}ag_{DATASET}_{kind}_{epoch}``."""
    os.makedirs(directory, exist_ok=True)
    tag = f"mix{m['att_speech_layer'].mode}ag_{config.DATASET}"
    paths = {}
    for mod, kind in (('mix_speech_multiEmbedding', 'emblayer'), ('mix_hidden_layer_3d', 'hidden3d'),
                      ('att_speech_layer', 'attlayer'), ('adjust_layer', 'adjlayer')):
        paths[kind] = os.path.join(directory, f"param_{tag}_{kind}_{epoch_idx}")
        torch.save({k: v.detach().cpu() for k, v in m[mod].state_dict().items()}, paths[kind])
    paths['dislayer'] = checkpoint.save_reference_discriminator(m['dis_layer'], tag, epoch_idx, directory)
    return paths


def main(max_epoch=None, max_batches=None, log=print, save_dir="params"):
    """dis.py:486-665 (training); ``max_epoch`` / ``max_batches`` bound a run."""
    np.random.seed(1)
    torch.manual_seed(1)
    random.seed(1)
    spk_global_gen = prepare_data(mode='global', train_or_test='train')
    global_para = next(spk_global_gen)
    spk_all_list, dict_spk2idx, dict_idx2spk, mix_speech_len, speech_fre, total_frames, spk_num_total, \
        batch_total = global_para
    del spk_global_gen
    num_labels = len(spk_all_list)
    m, optimizer = build(speech_fre, mix_speech_len, num_labels, spk_num_total)
    lr_sched = schedule.evalver(optimizer.param_groups[0]['lr'])  # :543-547, the EvalVer halving
    history = []
    for epoch_idx in range(config.MAX_EPOCH if max_epoch is None else max_epoch):
        lr_data = lr_sched.at_epoch_start(epoch_idx)
        for ee in optimizer.param_groups:
            ee['lr'] = lr_data
        lrs.send('lr', lr_data)
        train_data_gen = prepare_data('once', 'train')
        batch_idx = 0
        while True:
            train_data = next(train_data_gen)
            if train_data is False:
                break
            out = train_step(m, optimizer, train_data, dict_spk2idx, dict_idx2spk, num_labels)
            history.append((float(out['loss']), float(out['loss_dis'])))
            log(f"epoch {epoch_idx} batch {batch_idx} loss {history[-1][0]:.6f} loss_dis {history[-1][1]:.6f} "
                f"acc_dis {out['acc_dis']:.3f} lr {lr_data:g}")
            batch_idx += 1
            if max_batches is not None and batch_idx >= max_batches:
                break
        if epoch_idx >= 10 and epoch_idx % 5 == 0:  # :649-662
            save_params(m, epoch_idx, save_dir)
    return m, history


if __name__ == "__main__":
    main()
