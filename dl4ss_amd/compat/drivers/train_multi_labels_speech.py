"""py3 mirror of ``main`` of ``Torch_multi/test_multi_labels_speech.py`` (:354-465) -- training the
speaker classifier: BiLSTM(129, 2 HIDDEN_UNITS, 3 layers) -> mean over t -> Linear -> sigmoid (:235-273),
``MultiLabelSoftMarginLoss`` on the sigmoid output (:397,437), Adam(lr=1e-5) halved at every epoch with
``epoch_idx % 50 == 0`` -- epoch 0 included (:395,405-407) -- and a state_dict saved when
``epoch_idx > 10 and epoch_idx % 5 == 0`` (:447-449).  Imports the reference's names (``config``,
``predata_multiAims``, ``myNet``, ``test_multi_labels_speech`` -- whose ``count_multi_acc`` is restated in
``compat/multi_labels_acc.py`` and exported under the reference's module name by ``compat.install()``); the
step runs on
``myNet.MIX_SPEECH_classifier`` through torch autograd (HIP kernels underneath: the large-hidden BPTT
behind ``dl4ss::birnn_layer_bwd``) with the HIP Adam.  The fused single-call step is
``dl4ss_amd.classifier.ClassifierTrainer``."""
import os
import random

import numpy as np
import torch

from dl4ss_amd import compat as _compat

_compat.install()

import config  # noqa: E402
from predata_multiAims import prepare_data, prepare_datasize, prepare_data_fake  # noqa: E402,F401
import myNet  # noqa: E402
from test_multi_labels_speech import multi_label_vector, count_multi_acc  # noqa: E402

from dl4ss_amd.compat.optim import Adam  # noqa: E402
from dl4ss_amd.compat.drivers import _common as C  # noqa: E402
from dl4ss_amd import schedule  # noqa: E402


class MIX_SPEECH_classifier(myNet.MIX_SPEECH_classifier):
    """test_multi_labels_speech.py:235-273: nn.LSTM(input_fre, 2 HIDDEN_UNITS, 3 layers, bidirectional)."""

    def __init__(self, input_fre, mix_speech_len, num_labels):
        super().__init__(input_fre, mix_speech_len, num_labels, hidden=2 * config.HIDDEN_UNITS, num_layers=3,
                         precision=getattr(config, "PRECISION", "fp32"))


def build(speech_fre, mix_speech_len, num_labels):
    m = dict(mix_speech_class=MIX_SPEECH_classifier(speech_fre, mix_speech_len, num_labels).to(C.dev()))
    optimizer = Adam([{'params': m['mix_speech_class'].parameters()}], lr=0.00001)
    return m, optimizer


loss_func = torch.nn.MultiLabelSoftMarginLoss()


def train_step(m, optimizer, train_data, dict_spk2idx):
    """test_multi_labels_speech.py:416-445 on one batch dict."""
    mix_speech = m['mix_speech_class'](C.cuda(train_data['mix_feas']))
    y_spk, y_map = multi_label_vector(train_data['multi_spk_fea_list'], dict_spk2idx)
    y_out_batch = mix_speech.detach().cpu().numpy()
    acc1, acc2, all_num_batch, all_line_batch, recall_rate = count_multi_acc(y_out_batch, y_spk, alpha=-0.1,
                                                                             top_k_num=2)
    loss = loss_func(mix_speech, C.cuda(y_map))
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return dict(loss=loss.detach(), prob=mix_speech.detach(), acc_all=acc1, acc_line=acc2, recall_rate=recall_rate)


def save_path(epoch_idx):
    return 'params/param_speech_123onezeroag5dropout_{}_multilabel_epoch{}'.format(config.DATASET, epoch_idx)


def main(max_epoch=None, max_batches=None, log=print):
    np.random.seed(1)
    torch.manual_seed(1)
    random.seed(1)
    spk_all_list, dict_spk2idx, dict_idx2spk, mix_speech_len, speech_fre, total_frames, spk_num_total = \
        next(prepare_data(mode='global', train_or_test='train'))
    num_labels = len(spk_all_list)
    m, optimizer = build(speech_fre, mix_speech_len, num_labels)
    sched = schedule.classifier(optimizer.param_groups[0]['lr'])
    history = []
    n_batches = config.EPOCH_SIZE if max_batches is None else max_batches
    for epoch_idx in range(config.MAX_EPOCH if max_epoch is None else max_epoch):
        lr = sched.at_epoch_start(epoch_idx)
        for ee in optimizer.param_groups:
            ee['lr'] = lr
        acc_all, acc_line, recalls = 0., 0., []
        for batch_idx in range(n_batches):
            train_data = next(prepare_data('once', 'train'))
            out = train_step(m, optimizer, train_data, dict_spk2idx)
            acc_all += out['acc_all']
            acc_line += out['acc_line']
            recalls.append(out['recall_rate'])
            history.append(float(out['loss']))
            log(f"epoch {epoch_idx} batch {batch_idx} loss {history[-1]:.6f} recall {out['recall_rate']:.3f} lr {lr:g}")
        if config.Save_param and epoch_idx > 10 and epoch_idx % 5 == 0:
            os.makedirs('params', exist_ok=True)
            torch.save({k: v.detach().cpu() for k, v in m['mix_speech_class'].state_dict().items()},
                       save_path(epoch_idx))
        log(f"epoch {epoch_idx}: all elements acc {acc_all / max(n_batches, 1):.4f}, all sample acc "
            f"{acc_line / max(n_batches, 1):.4f}, recall {float(np.mean(recalls)) if recalls else float('nan'):.4f}")
    return m, history


if __name__ == "__main__":
    main()
