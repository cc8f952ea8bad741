"""MI355X-native greedy coded sampler (compression without quantization).

Public surface mirrors the reference's code/coded_greedy_sampler.py,
code/misc.py and code/binary_io.py (bit-string helpers); every sample is
computed by the gfx950 kernels in libcwq.so (see include/cwq.h).
"""
from .backfit import (backfit_blocks, backfit_blocks_var, code_grouped_greedy_sample_backfit,
                      code_grouped_greedy_sample_var_backfit, encode_blocks_backfit,
                      encode_blocks_var_backfit)
from .beam import (code_grouped_greedy_sample_beam, code_grouped_greedy_sample_var_beam,
                   encode_blocks_beam, encode_blocks_var_beam)
from .binary_io import (bitcode_to_indices, elias_delta_code, elias_delta_decode,
                        elias_delta_code_many, elias_delta_decode_many,
                        from_bit_string, indices_to_bitcode, read_bin_code, to_bit_string,
                        write_bin_code)
from .coding import ArithmeticCoder
from .coded_greedy_sampler import (Normal, code_greedy_sample, code_grouped_greedy_sample,
                                   code_grouped_greedy_sample_batch,
                                   decode, decode_blocks, decode_greedy_sample,
                                   decode_grouped_greedy_sample,
                                   decode_grouped_greedy_sample_batch, encode, encode_blocks,
                                   encode_workspace_bytes, group_size_threshold, group_starts)
from .coded_importance_sampler import (code_grouped_importance_sample,
                                       code_grouped_importance_sample_batch,
                                       code_importance_sample,
                                       decode_grouped_importance_sample,
                                       decode_grouped_importance_sample_batch,
                                       decode_importance_sample, importance_decode_blocks,
                                       importance_encode_blocks)
from .misc import stateless_normal_sample
from .pln import ProbabilisticLadderNetwork, build_empirical_dists
from .parallel import gather_indices, shard_range
from .ratetable import (choose_bits, choose_bits_total, choose_bits_total_device,
                        code_grouped_greedy_sample_rate, encode_blocks_rate,
                        encode_blocks_rate_total, rate_table)
from .streaming import encode_blocks_host
from .varbits import (block_bits, code_grouped_greedy_sample_var, decode_blocks_var,
                      decode_grouped_greedy_sample_var, encode_blocks_var, pack_indices,
                      unpack_indices)

__all__ = [
    "Normal", "code_greedy_sample", "decode_greedy_sample", "code_grouped_greedy_sample",
    "decode_grouped_greedy_sample", "encode", "decode", "encode_blocks", "decode_blocks",
    "encode_workspace_bytes", "group_starts", "group_size_threshold",
    "stateless_normal_sample", "to_bit_string", "from_bit_string", "indices_to_bitcode",
    "bitcode_to_indices", "shard_range", "gather_indices", "elias_delta_code",
    "elias_delta_decode", "elias_delta_code_many", "elias_delta_decode_many",
    "code_importance_sample", "decode_importance_sample",
    "code_grouped_importance_sample", "decode_grouped_importance_sample",
    "code_grouped_importance_sample_batch",
    "importance_encode_blocks", "importance_decode_blocks", "ArithmeticCoder",
    "write_bin_code", "read_bin_code", "ProbabilisticLadderNetwork", "build_empirical_dists",
    "encode_blocks_host", "code_grouped_greedy_sample_batch",
    "decode_grouped_greedy_sample_batch", "decode_grouped_importance_sample_batch",
    "block_bits", "encode_blocks_var", "decode_blocks_var", "pack_indices", "unpack_indices",
    "code_grouped_greedy_sample_var", "decode_grouped_greedy_sample_var",
    "encode_blocks_beam", "code_grouped_greedy_sample_beam",
    "encode_blocks_var_beam", "code_grouped_greedy_sample_var_beam",
    "backfit_blocks", "encode_blocks_backfit", "code_grouped_greedy_sample_backfit",
    "backfit_blocks_var", "encode_blocks_var_backfit", "code_grouped_greedy_sample_var_backfit",
    "rate_table", "choose_bits", "choose_bits_total", "encode_blocks_rate",
    "choose_bits_total_device", "encode_blocks_rate_total", "code_grouped_greedy_sample_rate",
]
