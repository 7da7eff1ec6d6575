# tests/emu/fftconv_group_asan_main.cpp as a stand-alone program under AddressSanitizer + UBSan, for tests/test_emu_fftconv_group_asan.py: the host
# emulation of both forms of the grouped tile kernel (fftConv.groups: the sum form on complex tiles, the depthwise form on real tile pairs) and of the
# grouped pointwise multiply-accumulate pass on exactly sized heap blocks.  Same compiler and flags as Makefile's libmi355emu_asan.so rule, without
# -shared: the program has its own main and needs no preloaded runtime.
#   make -f fftconv_group_asan.mk && ASAN_OPTIONS=detect_leaks=0 ./fftconv_group_asan
CXX = /opt/rocm/lib/llvm/bin/clang++
CSRC = ../../webgpu-fft_amd/csrc
CXXFLAGS = -std=c++17 -O1 -g -DMI355_HOST_EMU -fPIC -pthread -I$(CSRC) -I../../include -Wall -Wno-unused-function
DEPS = $(wildcard $(CSRC)/*.hpp $(CSRC)/*.def $(CSRC)/*.inc) $(CSRC)/plan.cpp fftconv_group_asan_main.cpp

fftconv_group_asan: $(DEPS)
	$(CXX) $(CXXFLAGS) -fsanitize=address,undefined -fno-omit-frame-pointer -ftls-model=initial-exec fftconv_group_asan_main.cpp $(CSRC)/plan.cpp -o $@
