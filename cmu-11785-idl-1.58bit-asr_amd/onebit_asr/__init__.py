"""onebit_asr — MI355X-native BitLinear (1.58-bit QuantizedLinear) hot path for the
1.58-bit Conformer ASR training step of y00njaekim/CMU-11785-IDL-1.58bit-ASR.

Import path mirrors the reference (``from onebit_asr.conformer import ConformerASR``,
train.py:18). The BitLinear kernels live in ``libonebit_hip.so`` (C ABI:
include/onebit_hip.h), bound by ``onebit_asr._lib``.
"""
from .quant import BitLinear, QuantizedLinear, quantize_weight  # noqa: F401
from .infer import (attention_rescore, ctc_beam_search_batch_device,  # noqa: F401
                    ctc_beam_search_bias_device, ctc_beam_search_lm_device,
                    ctc_beam_search_nbest_device, seq_logprob)
from .bias import ContextBias, bias_seq_score, bias_step  # noqa: F401
from .frontend import FrontEnd, draw_specaug_starts, fbank_batch  # noqa: F401
from .attdec import attention_beam_search, joint_beam_search, seq_topk  # noqa: F401
from .align import ctc_forced_align, span_seconds, token_confidence  # noqa: F401
from .edit import edit_distance, mbr_select, nbest_edit_distance, nbest_oracle  # noqa: F401
from .mwer import mwer_ctc_loss, nbest_ctc_logprob  # noqa: F401
from .metrics import (attention_decode_batch, compute_wer, compute_wer_device,  # noqa: F401
                      ctc_attention_rescore_batch, ctc_beam_search, ctc_beam_search_batch,
                      ids_to_text, joint_decode_batch, levenshtein_distance, token_error_counts,
                      word_spans)

__version__ = "0.1.0"
