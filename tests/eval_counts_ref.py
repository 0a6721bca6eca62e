"""numpy restatement of the counting rule of src/evaluation.py:27-52 for any number of classes K (the reference, and
oracle.mcl_oracle.eval_compare after it, build the score tensor with 21 channels whatever num_cls is).  Every table is int64
[K][3] = (TP, P, T), the layout of the device tables."""
import numpy as np


def counts(predict, gt, K):
    """:38-50 for one image: predict, gt uint8 [H,W].  Pixels with gt == 255 are out; a gt in K..254 counts towards P only; a
    predict >= K counts nowhere."""
    predict, gt = np.asarray(predict), np.asarray(gt)
    cal = gt < 255
    mask = (predict == gt) * cal
    out = np.zeros((K, 3), np.int64)
    for i in range(K):
        out[i] = (np.sum((gt == i) * mask), np.sum((predict == i) * cal), np.sum((gt == i) * cal))
    return out


def dict_predict(predict_dict, threshold, K, shape=None):
    """:28-33 with K channels: channel 0 is the threshold, channel key + 1 the dict's map, absent channels 0; np.argmax (the first
    maximum wins).  shape: the image size, needed where the dict is empty."""
    h, w = shape if shape is not None else list(predict_dict.values())[0].shape
    tensor = np.zeros((K, h, w), np.float32)
    for key in predict_dict.keys():
        tensor[key + 1] = predict_dict[key]
    tensor[0, :, :] = threshold
    return np.argmax(tensor, axis=0).astype(np.uint8)


def dict_counts(predict_dict, gt, threshold, K):
    return counts(dict_predict(predict_dict, threshold, K, np.asarray(gt).shape), gt, K)


def curve_counts(predict_dict, gt, thresholds, K):
    """int64 [nt][K][3]: dict_counts at every threshold."""
    return np.stack([dict_counts(predict_dict, gt, np.float32(t), K) for t in thresholds])


def half_dict(pred, label):
    """The dict of the rapid evaluation (train_mcl.py:299-303): pred [K,H,W] fp32 already normalised, label [K]; channel k >= 1
    becomes key k - 1 with the values rounded to float16, as the script's np.half files hold them."""
    pred, label = np.asarray(pred, np.float32), np.asarray(label, np.float32)
    return {k - 1: (pred[k] * label[k]).astype(np.float16).astype(np.float32) for k in range(1, pred.shape[0])}
