"""Float64 numpy restatement of the dataset scaler, in this project's own words (what csrc/scaler.hip and the NORM
epilogue of the dB kernels must compute).

  statistics(x)          x: dB features (clips, ..., frames, n_mels) float32 -> (mean_, mean_of_square_): per band, the sum
                         of x and the sum of x * x over every clip and frame, divided by their number.  The square is a
                         FLOAT32 product (the reference squares a float32 array before any widening); both sums run in
                         float64.
  normalize(x, mean, std)  float32((float64(x) - mean) / std): numpy's promotion, then the cast to the tensor's float32.
"""
import numpy as np


def statistics(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    rows = x.reshape(-1, x.shape[-1])
    square = rows * rows                                   # float32
    assert square.dtype == np.float32
    n = rows.shape[0]
    return rows.sum(axis=0, dtype=np.float64) / n, square.sum(axis=0, dtype=np.float64) / n


def std_of(mean, mean_of_square):
    return np.sqrt(mean_of_square - mean ** 2)


def normalize(x, mean, std):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return ((x.astype(np.float64) - mean) / std).astype(np.float32)
