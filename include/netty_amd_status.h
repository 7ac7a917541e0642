/*
 * netty_amd_status.h — per-chunk status codes shared by the C-ABI (include/netty_amd.h)
 * and the CPU oracle (oracle/netty_oracle.c).
 *
 * Netty's codecs signal failure with Java exceptions; Netty's own JNI layer returns
 * negative errno-style ints that the Java side turns into exceptions
 * (transport-native-unix-common/src/main/c/netty_unix_filedescriptor.c:115-117 →
 * FileDescriptor.java:105-110).  This build follows that convention: every batch entry
 * point writes one int32 status per chunk, >= 0 on success, < 0 = one of the codes below.
 * Each code maps 1:1 to a reference throw site (file:line relative to
 * codec-compression/src/main/java/io/netty/handler/codec/compression/).
 */
#ifndef NETTY_AMD_STATUS_H
#define NETTY_AMD_STATUS_H

#define NX_OK 0

/* Snappy.java:414-416  "Preamble is greater than 4 bytes" */
#define NX_ERR_SNAPPY_PREAMBLE_TOO_LONG   (-1)
/* Snappy.java:638-640  "Offset is less than minimum permissible value" */
#define NX_ERR_SNAPPY_OFFSET_ZERO         (-2)
/* Snappy.java:642-645  "Offset is greater than maximum value supported by this implementation" */
#define NX_ERR_SNAPPY_OFFSET_NEGATIVE     (-3)
/* Snappy.java:647-649  "Offset exceeds size of chunk" */
#define NX_ERR_SNAPPY_OFFSET_BEYOND       (-4)
/* SnappyFrameDecoder.java:203 buffer(…, 65536) max capacity → IndexOutOfBoundsException */
#define NX_ERR_SNAPPY_OUTPUT_OVERFLOW     (-5)
/* Snappy.java:480-492: code-63 literal length negative as Java int → IllegalArgumentException */
#define NX_ERR_SNAPPY_LITERAL_LEN_INVALID (-6)
/* Snappy.java:700-706  "mismatching checksum: %x (expected: %x)" */
#define NX_ERR_SNAPPY_CRC_MISMATCH        (-7)

/* FastLz.java:412-416  "invalid level: %d (expected: %d or %d)" */
#define NX_ERR_FASTLZ_BAD_LEVEL           (-20)
/* FastLz.java:444-465: match bytes read past the readable input → IndexOutOfBoundsException */
#define NX_ERR_FASTLZ_INPUT_OOB           (-21)
/* FastLzFrameDecoder.java:160-164  originalLength/actual length mismatch */
#define NX_ERR_FASTLZ_LENGTH_MISMATCH     (-22)
/* FastLzFrameDecoder.java:171-179  "stream corrupted: mismatching checksum" */
#define NX_ERR_FASTLZ_CRC_MISMATCH        (-23)

/* LzfDecoder.java:205 → ChunkDecoder.decodeChunk throws on corrupt data (3rd-party) */
#define NX_ERR_LZF_CORRUPT                (-30)

/* Frame-level format errors raised by the host framing state machines (SnappyFrameDecoder.java:
 * 116-118,128-133,138-140,152-157,159-165,181-201; FastLzFrameDecoder.java:121-124;
 * LzfDecoder.java:120-122,134-137).  The handle's err_msg carries the reference message. */
#define NX_ERR_FRAME_CORRUPT              (-40)

/* Lz4FrameDecoder.java:203-217: the LZ4 decompressor's LZ4Exception ("Malformed input at %d",
 * lz4-java 1.8.0, third-party) → DecompressionException.  Raised for a block that reads past its
 * input, copies from before the output start (offset 0 or > bytes produced), or does not produce
 * exactly the frame's decompressedLength. */
#define NX_ERR_LZ4_MALFORMED              (-50)

/* Device LZ4 frame scan (nx_lz4_frame_scan_batch), one code per Lz4FrameDecoder throw site: */
/* :127-130  "unexpected block identifier" */
#define NX_ERR_LZ4_BAD_MAGIC              (-51)
/* :136-141  "invalid compressedLength: %d (expected: 0-%d)" */
#define NX_ERR_LZ4_COMPRESSED_LENGTH      (-52)
/* :143-149  "invalid decompressedLength: %d (expected: 0-%d)" */
#define NX_ERR_LZ4_DECOMPRESSED_LENGTH    (-53)
/* :150-156  "stream corrupted: compressedLength(%d) and decompressedLength(%d) mismatch" */
#define NX_ERR_LZ4_LENGTH_MISMATCH        (-54)
/* :209-213  "unexpected blockType: %d (expected: %d or %d)" */
#define NX_ERR_LZ4_BLOCK_TYPE             (-55)
/* :226-228 → CompressionUtil.checkChecksum  "stream corrupted: mismatching checksum: %d (expected: %d)" */
#define NX_ERR_LZ4_CHECKSUM_MISMATCH      (-56)
/* :160-162  "stream corrupted: checksum error" (end block with a non-zero checksum) */
#define NX_ERR_LZ4_END_CHECKSUM           (-57)
/* Lz4FrameEncoder.allocateBuffer (Lz4FrameEncoder.java:190-214): EncoderException "requested encode
 * buffer size (%d bytes) exceeds the maximum allowable size (%d bytes)" when the blocks of the pending
 * bytes need more than maxEncodeSize (nx_lz4_frame_encoder_error has the message). */
#define NX_ERR_LZ4_ENCODE_SIZE            (-58)
/* Lz4FrameEncoder.encode after close() (Lz4FrameEncoder.java:233-239): IllegalStateException "encode
 * finished and not enough space to write remaining data" when allocateBuffer(allowEmptyReturn) returned
 * EMPTY_BUFFER, i.e. the message's blocks need fewer than blockSize bytes (:216-218). */
#define NX_ERR_LZ4_ENCODE_FINISHED        (-59)

/* ZstdEncoder.allocateBuffer (ZstdEncoder.java:105-122): EncoderException "requested encode buffer size
 * (%d bytes) exceeds the maximum allowable size (%d bytes)" or "too much data to allocate a buffer for
 * compression" (nx_zstd_encoder_error has the message). */
#define NX_ERR_ZSTD_ENCODE_SIZE           (-80)
/* Zstandard frame decoding (nx_zstd_decode_batch[_ex], nx_zstd_frame_info, nx_zstd_next_frame,
 * nx_zstd_decode_host[_ex], nx_zstd_decoder_decode).  zstd-jni turns every libzstd error into a ZstdException
 * that ZstdDecoder.java wraps in DecompressionException; the codes follow libzstd's error names. */
#define NX_ERR_ZSTD_WINDOW                (-81)  /* frameParameter_windowTooLarge: Window_Size or content size above 128 MiB */
#define NX_ERR_ZSTD_DICTIONARY            (-82)  /* dictionary_wrong: the frame names a dictionary (Dictionary_ID != 0) */
#define NX_ERR_ZSTD_CHECKSUM_UNSUPPORTED  (-83)  /* Content_Checksum flag set: refused by the entry points without VERIFY_CHECKSUM */
#define NX_ERR_ZSTD_MAGIC                 (-84)  /* prefix_unknown: not a Zstandard frame (skippable frames included) */
#define NX_ERR_ZSTD_TRUNCATED             (-85)  /* srcSize_wrong: the input ends inside the frame (frame_info: more input needed) */
#define NX_ERR_ZSTD_CORRUPT               (-86)  /* corruption_detected */
#define NX_ERR_ZSTD_OUTPUT_FULL           (-87)  /* dstSize_tooSmall: the regenerated bytes do not fit out_cap */
#define NX_ERR_ZSTD_CHECKSUM              (-88)  /* checksum_wrong: XXH64 of the regenerated bytes is not the frame's Content_Checksum */

/* Bzip2 stream decoding (nx_bzip2_decode_batch, nx_bzip2_decode_host, nx_bzip2_stream_info), one code per
 * throw site of Bzip2Decoder.java and its helpers, with the DecompressionException's message as the status
 * string.  Bzip2BlockDecompressor.java:234-237 ("block length exceeds max block length") has no code: the
 * declared-size checks at :206 and :223 keep a block at or below 900 000 bytes, so it cannot be reached. */
/* Bzip2Decoder.java:108-111  "Unexpected stream identifier contents. Mismatched bzip2 protocol version?" */
#define NX_ERR_BZIP2_STREAM_ID            (-110)
/* Bzip2Decoder.java:113-115  "block size is invalid" */
#define NX_ERR_BZIP2_BLOCK_SIZE           (-111)
/* Bzip2Decoder.java:131-133  "stream CRC error" */
#define NX_ERR_BZIP2_STREAM_CRC           (-112)
/* Bzip2Decoder.java:137-139  "bad block header" */
#define NX_ERR_BZIP2_BLOCK_HEADER         (-113)
/* Bzip2Decoder.java:186-188  "incorrect huffman groups number" */
#define NX_ERR_BZIP2_HUFFMAN_GROUPS       (-114)
/* Bzip2Decoder.java:190-192  "incorrect alphabet size" */
#define NX_ERR_BZIP2_ALPHABET             (-115)
/* Bzip2Decoder.java:201-203  "incorrect selectors number" */
#define NX_ERR_BZIP2_SELECTORS            (-116)
/* Bzip2HuffmanStageDecoder.java:178  "error decoding block": the groups outrun the selectors; also a
 * selector index at or above the table count (an array-index exception in the Java, a data error in libbz2) */
#define NX_ERR_BZIP2_DECODING_BLOCK       (-117)
/* Bzip2HuffmanStageDecoder.java:201  "a valid code was not recognised"; also a code length outside 1..23
 * and a code index outside the alphabet (array-index exceptions in the Java, data errors in libbz2) */
#define NX_ERR_BZIP2_CODE                 (-118)
/* Bzip2BlockDecompressor.java:207,224  "block exceeds declared block size" */
#define NX_ERR_BZIP2_BLOCK_EXCEEDS        (-119)
/* Bzip2BlockDecompressor.java:254  "start pointer invalid" */
#define NX_ERR_BZIP2_START_POINTER        (-120)
/* Bzip2BlockDecompressor.java:346  "block CRC error"; also a block whose inverse BWT closes before its last
 * byte (the reference walks the cycle again and then fails this check) */
#define NX_ERR_BZIP2_BLOCK_CRC            (-121)
/* This library's own: the input ends inside the stream (the reference waits for more input). */
#define NX_ERR_BZIP2_TRUNCATED            (-122)
/* This library's own: the decoded bytes do not fit out_cap. */
#define NX_ERR_BZIP2_OUTPUT_FULL          (-123)
/* This library's own: the block's randomised bit is set (the reference decodes such blocks; no encoder has
 * written one since bzip2 0.9.5). */
#define NX_ERR_BZIP2_RANDOMISED           (-124)
/* Bzip2 stream encoding (nx_bzip2_encode_batch, nx_bzip2_encode_host). */
/* Bzip2Encoder.java:98-101  "blockSizeMultiplier: %d (expected: 1-9)" (an IllegalArgumentException) */
#define NX_ERR_BZIP2_LEVEL                (-125)
/* This library's own: the stream does not fit the output slot. */
#define NX_ERR_BZIP2_ENCODE_FULL          (-126)
/* This library's own (nx_bzip2_encode_batch_split): the item's blocks fall beyond the call's max_blocks. */
#define NX_ERR_BZIP2_ENCODE_BLOCKS        (-127)
/* This library's own (nx_bzip2_scan_batch, nx_bzip2_decode_batch_split): the item holds more block and
 * end-of-stream magics than the call's max_blocks leaves room for. */
#define NX_ERR_BZIP2_DECODE_BLOCKS        (-128)
/* LZMA stream encoding (nx_lzma_encode_batch, nx_lzma_encode_host, LzmaFrameEncoder). */
/* LzmaFrameEncoder.java:139-147  "lc: %d (expected: 0-8)", "lp: %d (expected: 0-4)", "pb: %d (expected: 0-4)" (each an
 * IllegalArgumentException); from nx_lzma_encode_batch also lc + lp > 4, which the kernel's model does not hold */
#define NX_ERR_LZMA_PROPS                 (-140)
/* :157-159  "dictionarySize: %d (expected: 0+)" */
#define NX_ERR_LZMA_DICT_SIZE             (-141)
/* :160-164  "numFastBytes: %d (expected: 5-273)" */
#define NX_ERR_LZMA_FAST_BYTES            (-142)
/* This library's own: the stream does not fit the output slot. */
#define NX_ERR_LZMA_ENCODE_FULL           (-143)
/* Brotli stream encoding (nx_brotli_encode_batch, nx_brotli_encode_host, BrotliEncoder); the ranges are the ones
 * brotli4j's Encoder.Parameters accepts (setQuality, setWindow, setMode). */
/* "quality should be in range [0, 11], or -1" */
#define NX_ERR_BROTLI_QUALITY             (-150)
/* "lgwin should be in range [10, 24], or -1" */
#define NX_ERR_BROTLI_LGWIN               (-151)
/* mode: GENERIC (0), TEXT (1) or FONT (2) */
#define NX_ERR_BROTLI_MODE                (-152)
/* This library's own: the stream does not fit the output slot. */
#define NX_ERR_BROTLI_ENCODE_FULL         (-153)
/* Brotli stream decoding (nx_brotli_decode_batch, nx_brotli_decode_host; what brotli4j's DecoderJNI reports to
 * BrotliDecoder.java as ERROR): one code per format error of libbrotli's decoder (decode.h,
 * BROTLI_DECODER_ERROR_FORMAT_*), with the same meanings. */
#define NX_ERR_BROTLI_EXUBERANT_NIBBLE        (-154)  /* MLEN's last nibble is zero though MNIBBLES > 4 */
#define NX_ERR_BROTLI_RESERVED                (-155)  /* the reserved bit of a metadata meta-block is set */
#define NX_ERR_BROTLI_EXUBERANT_META_NIBBLE   (-156)  /* MSKIPLEN's last byte is zero though MSKIPBYTES > 1 */
#define NX_ERR_BROTLI_SIMPLE_HUFFMAN_ALPHABET (-157)  /* a simple code's symbol is outside the alphabet */
#define NX_ERR_BROTLI_SIMPLE_HUFFMAN_SAME     (-158)  /* a simple code names a symbol twice */
#define NX_ERR_BROTLI_CL_SPACE                (-159)  /* the code-length code is over- or under-subscribed */
#define NX_ERR_BROTLI_HUFFMAN_SPACE           (-160)  /* a prefix code is over- or under-subscribed */
#define NX_ERR_BROTLI_CONTEXT_MAP_REPEAT      (-161)  /* a zero run of a context map passes its end */
#define NX_ERR_BROTLI_BLOCK_LENGTH_1          (-162)  /* a command passes the end of the meta-block and reaches the end of libbrotli's ring buffer */
#define NX_ERR_BROTLI_BLOCK_LENGTH_2          (-163)  /* a command passes the end of the meta-block, short of the ring buffer's end */
#define NX_ERR_BROTLI_TRANSFORM               (-164)  /* a dictionary reference's transform index is 121 or more */
#define NX_ERR_BROTLI_DICTIONARY              (-165)  /* a dictionary reference with a copy length outside 4..24 */
#define NX_ERR_BROTLI_WINDOW_BITS             (-166)  /* WBITS 0010001, the large-window escape */
#define NX_ERR_BROTLI_PADDING_1               (-167)  /* non-zero padding before uncompressed or metadata bytes */
#define NX_ERR_BROTLI_PADDING_2               (-168)  /* non-zero padding after the last meta-block */
#define NX_ERR_BROTLI_DISTANCE                (-169)  /* a distance of zero or less from the ring, or above 0x7FFFFFFC */
/* This library's own: the input ends inside the stream (the reference waits for more input). */
#define NX_ERR_BROTLI_TRUNCATED               (-170)
/* This library's own: the decoded bytes do not fit out_cap. */
#define NX_ERR_BROTLI_OUTPUT_FULL             (-171)

/* Device frame scan (nx_snappy_frame_scan_batch), one code per SnappyFrameDecoder throw site: */
/* :116-118  "Unexpected length of stream identifier: %d" */
#define NX_ERR_SNAPPY_STREAM_ID_LENGTH        (-41)
/* :128-133 → checkByte :233-238  "Unexpected stream identifier contents. Mismatched snappy protocol version?" */
#define NX_ERR_SNAPPY_STREAM_ID_CONTENT       (-42)
/* :181-183  "Received COMPRESSED_DATA tag before STREAM_IDENTIFIER" */
#define NX_ERR_SNAPPY_COMPRESSED_BEFORE_ID    (-43)
/* :159-161  "Received UNCOMPRESSED_DATA tag before STREAM_IDENTIFIER" */
#define NX_ERR_SNAPPY_UNCOMPRESSED_BEFORE_ID  (-44)
/* :138-140  "Received RESERVED_SKIPPABLE tag before STREAM_IDENTIFIER" */
#define NX_ERR_SNAPPY_SKIPPABLE_BEFORE_ID     (-45)
/* :162-165  "Received UNCOMPRESSED_DATA larger than 65540 bytes" */
#define NX_ERR_SNAPPY_UNCOMPRESSED_TOO_LARGE  (-46)
/* :198-201  "Received COMPRESSED_DATA that contains uncompressed data that exceeds 65536 bytes" */
#define NX_ERR_SNAPPY_DECOMPRESSED_TOO_LARGE  (-47)
/* chunk length < 4: the checksum read runs past the chunk (:171-177, :194-195 throw from ByteBuf) */
#define NX_ERR_SNAPPY_CHUNK_TOO_SHORT         (-48)
/* :152-157  "Found reserved unskippable chunk type: 0x%x" */
#define NX_ERR_SNAPPY_UNSKIPPABLE             (-49)
/* Not an error: the frame scan's chunk list is full; the stream stopped before a data chunk and
 * continues from consumed[i] on the next call. */
#define NX_SCAN_LIST_FULL                     1

/* Device inflater (nx_inflate_batch) and JdkZlibDecoder: one code per error site of zlib's inflate()
 * (zlib 1.2.11 inflate.c, the library java.util.zip.Inflater wraps), with zlib's own text as the
 * status string.  JdkZlibDecoder.java:302-303 wraps each in DecompressionException("decompression
 * failure"). */
#define NX_ERR_INFLATE_BLOCK_TYPE         (-60)  /* "invalid block type" */
#define NX_ERR_INFLATE_STORED_LENGTHS     (-61)  /* "invalid stored block lengths" */
#define NX_ERR_INFLATE_TOO_MANY_SYMBOLS   (-62)  /* "too many length or distance symbols" */
#define NX_ERR_INFLATE_CODE_LENGTHS       (-63)  /* "invalid code lengths set" */
#define NX_ERR_INFLATE_BIT_LENGTH_REPEAT  (-64)  /* "invalid bit length repeat" */
#define NX_ERR_INFLATE_MISSING_EOB        (-65)  /* "invalid code -- missing end-of-block" */
#define NX_ERR_INFLATE_LITLEN_SET         (-66)  /* "invalid literal/lengths set" */
#define NX_ERR_INFLATE_DIST_SET           (-67)  /* "invalid distances set" */
#define NX_ERR_INFLATE_LITLEN_CODE        (-68)  /* "invalid literal/length code" */
#define NX_ERR_INFLATE_DIST_CODE          (-69)  /* "invalid distance code" */
#define NX_ERR_INFLATE_DISTANCE_TOO_FAR   (-70)  /* "invalid distance too far back" */
/* The zlib wrapper, checked by the handle on the host as inflate() does with nowrap = false: */
#define NX_ERR_ZLIB_HEADER_CHECK          (-71)  /* "incorrect header check" */
#define NX_ERR_ZLIB_DATA_CHECK            (-72)  /* "incorrect data check" (the Adler32 trailer) */
#define NX_ERR_ZLIB_METHOD                (-73)  /* "unknown compression method" */
#define NX_ERR_ZLIB_WINDOW                (-74)  /* "invalid window size" */
/* JdkZlibDecoder.java:276-280: a zlib stream that asks for a preset dictionary when none was given */
#define NX_ERR_ZLIB_NEED_DICT             (-75)
/* ZlibDecoder.java:74-81  "Decompression buffer has reached maximum size: %d" */
#define NX_ERR_ZLIB_MAX_ALLOCATION        (-76)
/* JdkZlibDecoder(dictionary) (:281): the stream's DICTID is not the Adler32 of the handle's dictionary.
 * Inflater.setDictionary throws IllegalArgumentException, which ByteToMessageDecoder wraps in
 * DecoderException (not DecompressionException).  The text is NOT pinned: zlib sets no message for this
 * error and no JVM run recorded Java's. */
#define NX_ERR_ZLIB_DICT_MISMATCH         (-77)
/* Not errors: why a stream of nx_inflate_batch stopped before the end of its final block. */
#define NX_INFLATE_NEED_INPUT             2
#define NX_INFLATE_OUTPUT_FULL            3

#define NX_ERR_INVALID_ARG                (-100)
#define NX_ERR_HIP                        (-101)
#define NX_ERR_NO_DEVICE                  (-102)
/* A kernel's own loop bound tripped (a bug guard: the kernel stopped instead of spinning). */
#define NX_ERR_INTERNAL                   (-103)

#endif
