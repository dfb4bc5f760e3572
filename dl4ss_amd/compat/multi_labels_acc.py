"""``count_multi_acc`` of Torch_multi/test_multi_labels_speech.py:300-351, the host-side (numpy) batch
statistics of the speaker-classifier training script.  (``multi_label_vector``, :285-298, is in
``compat/test_multi_labels_speech.py``, where ``compat.install()`` also exports this function: the reference's
``from test_multi_labels_speech import count_multi_acc`` resolves; the model and training loop, :235-273 / :354-465, are
``myNet.MIX_SPEECH_classifier`` / ``dl4ss_amd.classifier`` and the ``train_multi_labels_speech`` driver
mirror.)"""
import numpy as np


def count_multi_acc(y_out_batch, true_spk, alpha=0.5, top_k_num=3):
    """Batch statistics of the classifier output y_out_batch (B, N_lab) against the true speaker index
    lists -> (allelement_acc, allsample_acc, all_num, all_line, recall_rate), as the reference computes
    them (:300-351):

    * the predicted set of a row is its ``top_k_num`` largest entries (ids by descending value), or, with
      ``top_k_num`` 0, the entries above ``alpha``; ``recall_rate`` = predicted ids that are true / true ids;
    * the two accuracies keep the reference's arithmetic: it marks the TRUE ids in the row's prediction
      vector as well and compares that vector with an all-zero one, so ``allelement_acc`` is the share of
      labels neither predicted nor true, and ``allsample_acc`` the share of rows with no label at all."""
    all_line, len_vector = y_out_batch.shape
    all_num = all_line * len_vector
    if top_k_num:
        order = np.flip(np.argsort(y_out_batch), 1)[:, :top_k_num]
        predicted = [row for row in order]
        marks = np.zeros_like(y_out_batch)
        for k, row in enumerate(order):
            marks[k, row] = 1
    else:
        marks = np.int32(y_out_batch > alpha)
        predicted = [np.where(row == 1)[0] for row in marks]
    hits, num_all_true = 0., 0
    for pre, true in zip(predicted, true_spk):
        num_all_true += len(true)
        hits += sum(1 for one in pre if one in true)
    recall_rate = hits / num_all_true
    right_num = right_line = 0
    for k, true in enumerate(true_spk):
        for spk in true:
            marks[k, spk] = 1
        zeros = int(np.count_nonzero(marks[k] == 0))
        right_num += zeros
        right_line += int(zeros == len_vector)
    return float(right_num) / all_num, float(right_line) / all_line, all_num, all_line, recall_rate
