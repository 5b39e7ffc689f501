"""MI355X-native EnCodec / Mimi / DAC / WavTokenizer encode/decode paths behind the `audiocodecs.Codec` API."""

from .codec import Codec
from .config import DAC_16KHZ, DAC_24KHZ, DAC_44KHZ, DAC_TINY, ENCODEC_24KHZ, MIMI_24KHZ, MIMI_TINY, TINY, VOCOS_ENCODEC_24KHZ, VOCOS_TINY, WAVTOK_40, WAVTOK_75, WAVTOK_TINY, DacConfig, EncodecConfig, MimiConfig, VocosConfig, WavTokenizerConfig
from .dac import DAC
from .dnsmos import DNSMOS, DnsmosWeights, dnsmos, dnsmos_net, dnsmos_segments
from .encodec import Encodec, EncodecDecodeSessions, EncodecDecodeStream, EncodecEncodeSessions, EncodecEncodeStream
from .knn import KnnIndex, knn, knn_match
from .metrics import STOI, MelDistance, STFTDistance, spectral_distances, stoi
from .llama import IGNORE, LLAMA_TINY, LLAMA_TTS, LlamaConfig, LlamaDecoder, LlamaScore, stack_generated
from .mimi import Mimi, MimiDecodeSessions, MimiDecodeStream, MimiEncodeSessions, MimiEncodeStream
from .probe import PROBE_RECIPE, PROBE_TINY, ProbeConfig, ProbeOutput, TokenProbe
from .resample import ResampleSlots, ResampleStream
from .sampling import resample_tokens, sample_tokens
from .spksim import WAVLM_BASE_SV, WAVLM_SV_TINY, SpeakerEncoder, SpkSimWavLM, WavLMSVConfig, speaker_similarity
from .tokstats import CodebookUtil, TokenStatsState, codebook_stats, token_histogram
from .wavtokenizer import WavTokenizer

__all__ = ["Codec", "Encodec", "EncodecEncodeStream", "EncodecDecodeStream", "EncodecEncodeSessions", "EncodecDecodeSessions", "Mimi", "MimiEncodeStream", "MimiDecodeStream", "MimiEncodeSessions", "MimiDecodeSessions", "ResampleStream", "ResampleSlots", "knn_match", "knn", "KnnIndex", "spectral_distances", "STFTDistance", "MelDistance", "stoi", "STOI", "dnsmos", "dnsmos_net", "dnsmos_segments", "DnsmosWeights", "DNSMOS", "token_histogram", "codebook_stats", "TokenStatsState", "CodebookUtil", "sample_tokens", "resample_tokens", "LlamaDecoder", "LlamaConfig", "LlamaScore", "IGNORE", "LLAMA_TTS", "LLAMA_TINY", "stack_generated", "TokenProbe", "ProbeConfig", "ProbeOutput", "PROBE_TINY", "PROBE_RECIPE", "SpeakerEncoder", "speaker_similarity", "SpkSimWavLM", "WavLMSVConfig", "WAVLM_BASE_SV", "WAVLM_SV_TINY", "DAC", "WavTokenizer", "WavTokenizerConfig", "WAVTOK_40", "WAVTOK_75", "WAVTOK_TINY", "EncodecConfig", "MimiConfig", "DacConfig", "ENCODEC_24KHZ", "TINY", "MIMI_24KHZ", "MIMI_TINY",
           "DAC_44KHZ", "DAC_24KHZ", "DAC_16KHZ", "DAC_TINY", "VocosConfig", "VOCOS_ENCODEC_24KHZ", "VOCOS_TINY"]
__version__ = "0.1.0"
