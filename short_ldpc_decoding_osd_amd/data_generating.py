"""Test-frame generation and TFRecord writing with the reference's names
(LDPC_128/Testing_data_gen_128/data_generating.py:13-51, LDPC_128/Ldpc_128_testing/data_generating.py:8-26).
Host-side, not on the timed path: the benchmark generates its frames on the device."""
import numpy as np

from . import globalmap as GL
from .tfrecord import TFRecordWriter, encode_example, write_examples


def testing_data_generating(code, SNR, max_frame, rng=None):
    """AWGN frames: sigma = sqrt(1/(2 R 10^(SNR/10))), unit-mean channel, random message . G,
    BPSK 0 -> +1, NO 2/sigma^2 scaling (data_generating.py:13-51).  The reference draws from the
    unseeded global NumPy RNG (:10); pass ``rng`` (np.random.Generator) for reproducible sets."""
    n, k = code.check_matrix_column, code.k
    sigma = np.sqrt(1. / (2 * (float(k) / float(n)) * 10 ** (SNR / 10)))
    if GL.get_map('Rayleigh_fading', False):
        raise NotImplementedError("Rayleigh branch (data_generating.py:21-38): not on the host; testing_data_generating_device "
                                  "generates block-fading frames on the device")
    normal = rng.normal if rng is not None else np.random.normal
    integers = (lambda lo, hi, size: rng.integers(lo, hi, size=size)) if rng is not None else \
        (lambda lo, hi, size: np.random.randint(lo, hi, size=size))
    channel_information = normal(1, sigma, size=(max_frame, n))
    if not GL.get_map('ALL_ZEROS_CODEWORD_TESTING', False):
        rand_message = integers(0, 2, [max_frame, k])
        codewords = rand_message.dot(code.G) % 2
        testing_data = np.where(codewords == 0, channel_information, -channel_information)
        testing_data_labels = codewords.astype(np.int64)
    else:
        testing_data = channel_information
        testing_data_labels = np.zeros((max_frame, n), dtype=np.int64)
    return testing_data, testing_data_labels


def _device_channel():
    """The generator's channel keywords from the settings 'Rayleigh_fading' and 'duration' (a fading block lasts
    int(16 * duration) samples)."""
    rayleigh = bool(GL.get_map('Rayleigh_fading', False))
    return dict(rayleigh=rayleigh, fade_len=int(16 * GL.get_map('duration')) if rayleigh else 16)


def testing_data_generating_device(dec, SNR, max_frame, seed, frame0=0):
    """``testing_data_generating`` on the device (``dec``: a ``runtime.Decoder``): frames ``frame0 .. frame0 + max_frame - 1``
    of the counter-based set ``seed`` in one launch (ldpc_gen_frames).  Honours 'Rayleigh_fading', 'duration' and
    'ALL_ZEROS_CODEWORD_TESTING'.  Returns device tensors (y [max_frame, n] f32, label_bits [max_frame, words] int64 packed
    -- ``dec.unpack_bits`` gives one integer per bit).  The set is the generator's own (include/ldpc_osd.h), not NumPy's: it
    has the host function's distribution, not its draws.  Under Rayleigh fading it fades by global sample index, so every
    sample of every frame lies in a fading block: there is no zero tail after the last whole block."""
    return dec.gen_frames(max_frame, seed=seed, snr_db=SNR, mean=1.0, frame0=frame0,
                          all_zeros=bool(GL.get_map('ALL_ZEROS_CODEWORD_TESTING', False)), **_device_channel())


def get_tfrecords_example(feature, label):
    return encode_example(feature, label)


def make_tfrecord(data, out_filename):
    """One Example per row (data_generating.py:16-26)."""
    feats, labels = data
    write_examples(out_filename, feats, labels)


def _f_w(x, mid_sigma):
    return np.exp(-abs(x - mid_sigma))


def training_data_generating(code, SNRs, max_frame, rng=None):
    """Training frames (Training_data_gen_128/data_generating.py:41-81): for snr_lo != snr_hi the noise is scaled by the
    sigma and shifted by the mean of the exp(-|sigma - mid|)-weighted sigma density over [sigma1, sigma2] (scipy quad);
    for snr_lo == snr_hi sigma = sigma1 and mean 1.  Pass ``rng`` (np.random.Generator) for reproducible sets (the
    reference seeds the global NumPy RNG with 0)."""
    n, k = code.check_matrix_column, code.k
    randn = rng.standard_normal if rng is not None else (lambda size: np.random.randn(*size))
    integers = (lambda lo, hi, size: rng.integers(lo, hi, size=size)) if rng is not None else \
        (lambda lo, hi, size: np.random.randint(lo, hi, size=size, dtype=int))
    training_data_labels = np.zeros((max_frame, n), dtype=np.int64)
    noise = randn((max_frame, n))
    sigma, new_mean = _training_channel(n, k, SNRs)
    noise *= sigma
    noise += new_mean
    if GL.get_map('ALL_ZEROS_CODEWORD_TRAINING', False):
        training_data = noise
    else:
        codewords = integers(0, 2, [max_frame, k]).dot(code.G) % 2
        training_data = np.where(codewords == 0, noise, -noise)
        training_data_labels = codewords.astype(np.int64)
    return training_data, training_data_labels


def _training_channel(n, k, SNRs):
    """(sigma, mean) of a training set, as ``training_data_generating`` blends them over [snr_lo, snr_hi]."""
    from scipy import integrate

    SNR1, SNR2 = SNRs[0], SNRs[1]
    sig = lambda snr: np.sqrt(1. / (2 * (float(k) / float(n)) * 10 ** (snr / 10)))   # noqa: E731
    sigma1, sigma2, mid_sigma = sig(SNR1), sig(SNR2), sig((SNR1 + SNR2) / 2)
    if SNR1 != SNR2:
        tmp, _ = integrate.quad(_f_w, sigma1, sigma2, args=(mid_sigma,))
        weight_coefficient = 1 / tmp
        tmp_mean, _ = integrate.quad(lambda x, s: 2 / (x ** 2) * _f_w(x, s), sigma1, sigma2, args=(mid_sigma,))
        new_mean = weight_coefficient * tmp_mean
        tmp_variance, _ = integrate.quad(lambda x, s: 4 * (1 / (x ** 2) + 1 / (x ** 4)) * _f_w(x, s), sigma1, sigma2, args=(mid_sigma,))
        new_variance = weight_coefficient * tmp_variance - new_mean ** 2
        sigma = np.sqrt(new_variance)
    else:
        sigma, new_mean = sigma1, 1
    return sigma, new_mean


def training_data_generating_device(dec, SNRs, max_frame, seed, frame0=0):
    """``training_data_generating`` on the device: the blended sigma and mean are computed on the host exactly as there and
    handed to the generator (ldpc_gen_frames), which draws frames ``frame0 .. frame0 + max_frame - 1`` of the set ``seed``.
    Honours 'ALL_ZEROS_CODEWORD_TRAINING', 'Rayleigh_fading' and 'duration'.  Returns device tensors (y, packed label_bits)
    as ``testing_data_generating_device``."""
    sigma, new_mean = _training_channel(dec.n, dec.k, SNRs)
    return dec.gen_frames(max_frame, seed=seed, sigma=float(sigma), mean=float(new_mean), frame0=frame0,
                          all_zeros=bool(GL.get_map('ALL_ZEROS_CODEWORD_TRAINING', False)), **_device_channel())
