# Builds libsegan_hip.so (the C-ABI HIP library) in-tree for gfx950, and the oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := segan_pytorch_amd/csrc
SRCS := $(CSRC)/segan_api.hip $(CSRC)/segan_conv.hip $(CSRC)/segan_conv_edge.hip $(CSRC)/segan_wgrad.hip $(CSRC)/segan_pack.hip $(CSRC)/segan_conv_bf2.hip $(CSRC)/segan_wgrad_bf2.hip $(CSRC)/segan_pointwise.hip $(CSRC)/segan_stft.hip $(CSRC)/segan_snorm.hip $(CSRC)/segan_gemm.hip $(CSRC)/segan_audio.hip $(CSRC)/segan_quality.hip $(CSRC)/segan_bsseval.hip $(CSRC)/segan_srmr.hip $(CSRC)/segan_pitch.hip $(CSRC)/segan_pyin.hip $(CSRC)/segan_denoise.hip $(CSRC)/segan_omlsa.hip $(CSRC)/segan_rir.hip $(CSRC)/segan_dereverb.hip $(CSRC)/segan_stoi.hip $(CSRC)/segan_additive.hip $(CSRC)/segan_resample.hip $(CSRC)/segan_reverb.hip $(CSRC)/segan_distort.hip $(CSRC)/segan_whisper.hip $(CSRC)/segan_comm.hip
OBJS := $(SRCS:.hip=.o)
LIB := segan_pytorch_amd/libsegan_hip.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wall -Wno-unused-function

all: $(LIB)

$(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/segan_common.h $(CSRC)/segan_conv_shared.h $(CSRC)/segan_conv_tile.h $(CSRC)/segan_signal.h $(CSRC)/segan_stsa.h $(CSRC)/segan_fft_lds.h include/segan_hip.h include/segan_dereverb.h include/segan_pyin.h include/segan_omlsa.h include/segan_rir.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

clean:
	rm -f $(OBJS) $(LIB)

.PHONY: all clean
