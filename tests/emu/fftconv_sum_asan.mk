# tests/emu/fftconv_sum_asan_main.cpp as a stand-alone program under AddressSanitizer + UBSan, for tests/test_emu_fftconv_sum_asan.py: the host
# emulation of the tile kernel's sum over input channels (complex tiles and real tile pairs) and of the pointwise multiply-accumulate pass on exactly
# sized heap blocks.  Same compiler and flags as Makefile's libmi355emu_asan.so rule, without -shared: the program has its own main and needs no
# preloaded runtime.
#   make -f fftconv_sum_asan.mk && ASAN_OPTIONS=detect_leaks=0 ./fftconv_sum_asan
CXX = /opt/rocm/lib/llvm/bin/clang++
CSRC = ../../webgpu-fft_amd/csrc
CXXFLAGS = -std=c++17 -O1 -g -DMI355_HOST_EMU -fPIC -pthread -I$(CSRC) -I../../include -Wall -Wno-unused-function
DEPS = $(wildcard $(CSRC)/*.hpp $(CSRC)/*.def $(CSRC)/*.inc) $(CSRC)/plan.cpp fftconv_sum_asan_main.cpp

fftconv_sum_asan: $(DEPS)
	$(CXX) $(CXXFLAGS) -fsanitize=address,undefined -fno-omit-frame-pointer -ftls-model=initial-exec fftconv_sum_asan_main.cpp $(CSRC)/plan.cpp -o $@
