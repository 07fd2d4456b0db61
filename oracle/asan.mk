# ORACLE sanitizer build (host code only, CPU):  make -C oracle -f asan.mk
# clang rather than gcc so that the sanitizer line can state that it instruments no device code: -fno-gpu-sanitize
# (there is no device pass in this compile, so the flag does not change the output; clang notes it as unused).
CLANG ?= /opt/rocm/llvm/bin/clang
liboracle_asan.so: cdcl.c check.c oracle.h
	$(CLANG) -O1 -g -fsanitize=address,undefined -fno-gpu-sanitize -fPIC -std=c11 -D_POSIX_C_SOURCE=200809L -shared -o $@ cdcl.c check.c -lm
