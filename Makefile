# Build of the MI355X engine. `make` = the shipped gfx950 library; `make emu` = test-only emulator build.
# One object per translation unit (the kernels are split over kernels/launch_*.cpp), so `make -j` builds them in parallel.
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
CXX_EMU ?= $(ROCM)/lib/llvm/bin/clang++
CSRC := piper_amd/csrc
SRCS := $(CSRC)/engine.cpp $(CSRC)/engine_stream.cpp $(CSRC)/engine_deliver.cpp $(CSRC)/engine_pack.cpp $(CSRC)/engine_launch.cpp $(CSRC)/engine_issue.cpp $(CSRC)/kernels/launch_conv.cpp $(CSRC)/kernels/launch_bf3.cpp $(CSRC)/kernels/launch_front.cpp $(CSRC)/kernels/launch_tail.cpp \
        $(CSRC)/pe_api.cpp $(CSRC)/policy.cpp $(CSRC)/weights.cpp $(CSRC)/onnx_reader.cpp $(CSRC)/piper_shim.cpp
HDRS := include/piper.hpp $(CSRC)/engine.h $(CSRC)/engine_buffers.h $(CSRC)/engine_internal.h $(wildcard $(CSRC)/kernels/*.h) $(CSRC)/pe_rt.h $(CSRC)/policy.h $(CSRC)/weights.h \
        $(CSRC)/unicode_tables.h include/piper_hip.h
LIB := piper_amd/libpiper_hip.so
EMULIB := tests/emu/libpiper_hip_emu.so
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -Wno-unused-result -Wno-unused-value
EMUFLAGS := -DPE_EMU -O2 -mfma -mf16c -std=c++17 -Wno-psabi -fPIC -Itests/emu
# Leading scalar kernel parameters arrive in SGPRs at wave launch (up to 14 dwords): the launch units whose kernels are written
# for it (pe_rt.h PE_ENTRY_BATCH; scripts/entry_waits.py shows what each kernel gets)
PRELOAD := -mllvm -amdgpu-kernarg-preload-count=14
PRELOAD_UNITS := kernels/launch_front kernels/launch_conv kernels/launch_tail
OBJ := $(patsubst $(CSRC)/%.cpp,build/gfx950/%.o,$(SRCS))
OBJ_STAMPS := $(patsubst $(CSRC)/%.cpp,build/stamps/%.o,$(SRCS))
OBJ_EMU := $(patsubst $(CSRC)/%.cpp,build/emu/%.o,$(SRCS)) build/emu/hip_emu.o

all: $(LIB)
$(foreach u,$(PRELOAD_UNITS),build/gfx950/$(u).o build/stamps/$(u).o): HIPFLAGS += $(PRELOAD)

build/gfx950/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC $(OBJ) -o $@

emu: $(EMULIB)
build/emu/%.o: $(CSRC)/%.cpp $(HDRS) $(wildcard tests/emu/*.h)
	@mkdir -p $(dir $@)
	$(CXX_EMU) $(EMUFLAGS) -c $< -o $@
build/emu/hip_emu.o: tests/emu/hip_emu.cpp tests/emu/hip_emu.h
	@mkdir -p $(dir $@)
	$(CXX_EMU) $(EMUFLAGS) -c $< -o $@
# (linked beside the target and moved into place: tests that find no library run `make emu` themselves, several at once)
$(EMULIB): $(OBJ_EMU)
	$(CXX_EMU) -shared -fPIC $(OBJ_EMU) -o $(@D)/tmp$$$$.$(@F) && mv -f $(@D)/tmp$$$$.$(@F) $@

# tuning build: the same library with phase timestamps in the small kernels (scripts/stamps.py); never shipped
stamps: piper_amd/libpiper_hip_stamps.so
build/stamps/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -DPE_STAMPS -c $< -o $@
piper_amd/libpiper_hip_stamps.so: $(OBJ_STAMPS)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC $(OBJ_STAMPS) -o $@

# C++ callers of the piper:: API (mirror of the reference's test.cpp)
tests/cpp/test_piper: tests/cpp/test_piper.cpp $(LIB) include/piper.hpp
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_piper.cpp -o $@ -Lpiper_amd -lpiper_hip -Wl,-rpath,'$$ORIGIN/../../piper_amd'
tests/cpp/test_piper_emu: tests/cpp/test_piper.cpp $(EMULIB) include/piper.hpp
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_piper.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::targetLufs through the piper:: API (tests/test_loudness_cpp.py)
tests/cpp/test_loudness: tests/cpp/test_loudness.cpp $(LIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_loudness.cpp -o $@ -Lpiper_amd -lpiper_hip -Wl,-rpath,'$$ORIGIN/../../piper_amd'
tests/cpp/test_loudness_emu: tests/cpp/test_loudness.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_loudness.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::truePeak through the piper:: API (tests/test_true_peak_cpp.py)
tests/cpp/test_true_peak: tests/cpp/test_true_peak.cpp $(LIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_true_peak.cpp -o $@ -Lpiper_amd -lpiper_hip -Wl,-rpath,'$$ORIGIN/../../piper_amd'
tests/cpp/test_true_peak_emu: tests/cpp/test_true_peak.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_true_peak.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::limiter through the piper:: API (tests/test_limiter_cpp.py)
tests/cpp/test_limiter: tests/cpp/test_limiter.cpp $(LIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_limiter.cpp -o $@ -Lpiper_amd -lpiper_hip -Wl,-rpath,'$$ORIGIN/../../piper_amd'
tests/cpp/test_limiter_emu: tests/cpp/test_limiter.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_limiter.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::seed through the piper:: API (tests/test_seeds_emu.py)
tests/cpp/test_seeds_emu: tests/cpp/test_seeds.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_seeds.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::speakerBlend / ::speakerVector through the piper:: API (tests/test_speaker_blend_emu.py)
tests/cpp/test_speaker_blend_emu: tests/cpp/test_speaker_blend.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_speaker_blend.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'
# SynthesisConfig::sampleFormat through the piper:: API (tests/test_g711_cpp.py)
tests/cpp/test_g711: tests/cpp/test_g711.cpp $(LIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_g711.cpp -o $@ -Lpiper_amd -lpiper_hip -Wl,-rpath,'$$ORIGIN/../../piper_amd'
tests/cpp/test_g711_emu: tests/cpp/test_g711.cpp $(EMULIB) include/piper.hpp include/piper_hip.h
	g++ -O1 -std=c++17 -Iinclude tests/cpp/test_g711.cpp -o $@ -Ltests/emu -lpiper_hip_emu -Wl,-rpath,'$$ORIGIN/../emu'

clean:
	rm -rf build $(LIB) $(EMULIB) tests/cpp/test_piper tests/cpp/test_piper_emu tests/cpp/test_loudness tests/cpp/test_loudness_emu \
	       tests/cpp/test_true_peak tests/cpp/test_true_peak_emu tests/cpp/test_limiter tests/cpp/test_limiter_emu \
	       tests/cpp/test_seeds_emu tests/cpp/test_speaker_blend_emu tests/cpp/test_g711 tests/cpp/test_g711_emu
.PHONY: all emu stamps clean
